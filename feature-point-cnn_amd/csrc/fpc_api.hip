// fpc_api.hip -- the C-ABI of include/fpc.h: context, weight packing, launch plan.
//
// Data layout in HBM (all fp32): activations NHWC with the channel count padded to a
// multiple of 8 (65 -> 72); one buffer per tensor of the network sized for max_batch
// frames; the transposed-conv output and the encoder features share ONE 256-channel
// buffer (`cat`), so torch.cat (python/src/superpoint.py:59) costs nothing; weights
// live in one packed blob (BN folded, MFMA fragment order) that stays L2-resident.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/fpc.h"
#include "block_mfma.h"
#include "block_bf16.h"
#include "convt_bf16.h"
#include "block_x3.h"
#include "stem_bf16.h"
#include "wblock_mfma.h"
#include "wblock16_mfma.h"
#include "wblock36_mfma.h"
#include "wblock36p_mfma.h"
#include "conv_mfma.h"
#include "kernels_misc.h"
#include "queue_map.h"
#include "match.h"
#include "match_frames.h"
#include "match_bank.h"
#include "match_bank_bf16.h"
#include "match_guided.h"
#include "match_guided_cells.h"
#include "match_guided_epipolar.h"
#include "match_guided_pose.h"
#include "ransac_homography.h"
#include "ransac_fundamental.h"
#include "pose_epipolar.h"
#include "pose_homography.h"
#include "match_bank_topk.h"
#include "pnp_ransac.h"
#include "sim3_ransac.h"
#include "p3p_ransac.h"
#include "essential_ransac.h"
#include "landmarks.h"
#include "refine_pose.h"
#include "refine_window.h"
#include "pose_graph.h"
#include "homography.h"
#include "weights.h"
#include "plan_options.h"

namespace fpc {

constexpr int BLOB_HEADER_FLOATS = 16;
constexpr uint32_t BLOB_MAGIC = 0x57435046u;   // "FPCW"

static thread_local std::string g_hip_err;

#define HIPCHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      g_hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
      return FPC_E_HIP;                                                                  \
    }                                                                                    \
  } while (0)

// ------------------------------------------------------------------------------------
// Kernel instances.  Each X-macro list below is the one place an instance is declared: it expands once into its
// enumerator and once into its table row.  New instances go at the END of a list, and a new Winograd list behind the
// others: plan_hash mixes the enumerators.
// ------------------------------------------------------------------------------------
template <auto Kernel, int Threads, int Lds, typename Args>
static void launch_as(const Args& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(Kernel, grid, dim3(Threads), Lds, st, a);
}

// What the host needs to launch one instance, and the head of every table row
template <typename Args>
struct Instance {
  const void* fn;
  int lds_bytes, threads;
  void (*launch)(const Args&, dim3, hipStream_t);
};
template <auto Kernel, typename Cfg, int Threads, typename Args>
static Instance<Args> instance_of() {
  return {(const void*)Kernel, Cfg::LDS_BYTES, Threads, launch_as<Kernel, Threads, Cfg::LDS_BYTES, Args>};
}

// KIND(name, TH,TW, S,EXT, KC, WM,WN, MB,NB)
#define FPC_KINDS(X)                                                        \
  X(T816_3x3_K64_N64, 8, 16, 1, 3, 64, 4, 1, 1, 2)                          \
  X(T816_1x1_K64_N64, 8, 16, 1, 1, 64, 4, 1, 1, 2)                          \
  X(T620_3x3s2_K32_N128, 6, 20, 2, 3, 32, 2, 2, 2, 2)                       \
  X(T620_3x3_K64_N128, 6, 20, 1, 3, 64, 2, 2, 2, 2)                         \
  X(T620_1x1_K64_N128, 6, 20, 1, 1, 64, 2, 2, 2, 2)                         \
  X(T620_2x2_K64_N128, 6, 20, 1, 2, 64, 2, 2, 2, 2)                         \
  X(T320_2x2_K64_N128, 3, 20, 1, 2, 64, 1, 4, 2, 1)                         \
  X(T320_1x1_K64_N128, 3, 20, 1, 1, 64, 1, 4, 2, 1)                         \
  X(T620_3x3_K64_N96, 6, 20, 1, 3, 64, 4, 1, 1, 3)                          \
  X(T620_1x1_K64_N96, 6, 20, 1, 1, 64, 4, 1, 1, 3)                          \
  X(T620_3x3_K72_N96, 6, 20, 1, 3, 72, 4, 1, 1, 3)                          \
  X(T620_1x1_K72_N96, 6, 20, 1, 1, 72, 4, 1, 1, 3)

enum Kind {
#define X(name, ...) K_##name,
  FPC_KINDS(X)
#undef X
      K_COUNT
};

struct KindInfo : Instance<ConvArgs> {
  const char* name;
  const char* symbol;   // as rocprofv3 prints it
  int TH, TW, S, EXT, KC, WM, WN, MB, NB;
};

static const KindInfo g_kinds[K_COUNT] = {
#define X(name, TH, TW, S, EXT, KC, WM, WN, MB, NB)                                                                                      \
  {instance_of<conv_mfma_kernel<TH, TW, S, EXT, KC, WM, WN, MB, NB>, ConvCfg<TH, TW, S, EXT, KC, WM, WN, MB, NB>, WM * WN * 64, ConvArgs>(), \
   #name, "conv_mfma_kernel<" #TH ", " #TW ", " #S ", " #EXT ", " #KC ", " #WM ", " #WN ", " #MB ", " #NB ">", TH, TW, S, EXT, KC, WM, WN, MB, NB},
    FPC_KINDS(X)
#undef X
};

// conv2_mfma_kernel (conv_mfma.h: the same convolution with a quarter of the VALU instructions) for the two
// instances of the default fp32 plan -- the ConvTranspose phases and descriptor.layer_in.1's 1x1; launches it does not
// cover (a second K source, workgroups that store only part of their N channels) and every other instance keep
// conv_mfma_kernel.
#define FPC_LEAN_KINDS(X)                          \
  X(T320_2x2_K64_N128, 3, 20, 1, 2, 64, 1, 4, 2, 1) \
  X(T320_1x1_K64_N128, 3, 20, 1, 1, 64, 1, 4, 2, 1)
struct LeanKindInfo : Instance<ConvArgs> {
  Kind kind;
  const char* symbol;
};
static const LeanKindInfo g_lean_kinds[] = {
#define X(name, TH, TW, S, EXT, KC, WM, WN, MB, NB)                                                                                        \
  {instance_of<conv2_mfma_kernel<TH, TW, S, EXT, KC, WM, WN, MB, NB>, Conv2Cfg<TH, TW, S, EXT, KC, WM, WN, MB, NB>, WM * WN * 64, ConvArgs>(), \
   K_##name, "conv2_mfma_kernel<" #TH ", " #TW ", " #S ", " #EXT ", " #KC ", " #WM ", " #WN ", " #MB ", " #NB ">"},
    FPC_LEAN_KINDS(X)
#undef X
};
static const LeanKindInfo* lean_kind(Kind k) {
  for (const LeanKindInfo& l : g_lean_kinds)
    if (l.kind == k) return &l;
  return nullptr;
}

// Fused ResNetBlock instances.  BKIND(name, TH,TW, S, KC, WM,WN, MB,NB, CMIDP)
#define FPC_BLOCK_KINDS(X)                                   \
  X(B816_s1_K64_C64, 8, 16, 1, 64, 4, 1, 1, 2, 64)           \
  X(B1616_s1_K32_C64, 16, 16, 1, 32, 4, 1, 2, 2, 64)         \
  X(B620_s2_K32_C128, 6, 20, 2, 32, 2, 2, 2, 2, 128)         \
  X(B620_s1_K64_C128, 6, 20, 1, 64, 2, 2, 2, 2, 128)         \
  X(B620_s1_K64_C72, 6, 20, 1, 64, 4, 1, 1, 3, 72)           \
  X(B620_s1_K72_C72, 6, 20, 1, 72, 4, 1, 1, 3, 72)           \
  X(B320_s2_K32_C256, 3, 20, 2, 32, 1, 4, 2, 2, 256)         \
  X(B310_s2_K32_C256, 3, 10, 2, 32, 1, 4, 1, 2, 256)         \
  X(B320_s2_K32_C128, 3, 20, 2, 32, 1, 4, 2, 1, 128)         \
  X(B320_s1_K64_C256, 3, 20, 1, 64, 1, 4, 2, 2, 256)         \
  X(B416_s2_K32_C128, 4, 16, 2, 32, 1, 4, 2, 1, 128)
// (B416_s2_K32_C128: B320_s2_K32_C128's fragments on 64 pixels that fill the M = 64 rows -- retile_rows below.)

enum BKind {
#define X(name, ...) BK_##name,
  FPC_BLOCK_KINDS(X)
#undef X
      BK_COUNT
};

struct BKindInfo : Instance<BlockArgs> {
  const char* name;
  const char* symbol;
  int TH, TW, S, KC, WM, WN, MB, NB, CMIDP;
};

static const BKindInfo g_bkinds[BK_COUNT] = {
#define X(name, TH, TW, S, KC, WM, WN, MB, NB, CMIDP)                                                                                            \
  {instance_of<block_mfma_kernel<TH, TW, S, KC, WM, WN, MB, NB, CMIDP>, BlockCfg<TH, TW, S, KC, WM, WN, MB, NB, CMIDP>, WM * WN * 64, BlockArgs>(), \
   #name, "block_mfma_kernel<" #TH ", " #TW ", " #S ", " #KC ", " #WM ", " #WN ", " #MB ", " #NB ", " #CMIDP ">", TH, TW, S, KC, WM, WN, MB, NB, CMIDP},
    FPC_BLOCK_KINDS(X)
#undef X
};

// Winograd ResNetBlock instances.  WKIND(name, KC, NBT, CMID): wblock_mfma_kernel (generation 1: 32x32x2 blocks, a wave
// owns 4 positions x 64 channels, phases in lockstep); W16KIND(name, NCG): wblock16_kernel (generation 2: 16x16x4 blocks,
// a wave owns 16 channels x all positions, input side pipelined into the GEMM), N = 16 NCG output channels.
#define FPC_WBLOCK_KINDS(X)     \
  X(W816_K32_C64, 32, 2, 64)    \
  X(W816_K32_C128, 32, 4, 128)  \
  X(W816_K32_C72, 32, 3, 72)    \
  X(W816_K24_C72, 24, 3, 72)
#define FPC_W16_KINDS(X) \
  X(W16_C64, 4, 8)       \
  X(W16_C128, 8, 8)      \
  X(W16_C128H, 8, 4)
// W36KIND(name, NB, TYT, TXT): wblock36_kernel (generation 3: Winograd F(4x4,3x3), one wave per SIMD, 16 Winograd tiles
// of 4x4 pixels arranged TYT x TXT per workgroup), N = 64 NB output channels.
#define FPC_W36_KINDS(X) \
  X(W36_C64_4x4, 1, 4, 4)  \
  X(W36_C64_2x8, 1, 2, 8)  \
  X(W36_C128_4x4, 2, 4, 4) \
  X(W36_C128_2x8, 2, 2, 8)

// W36PKIND(name, TYT, TXT): wblock36p_kernel (round 5: the 64-channel instance at TWO waves per SIMD -- 512 threads, the 36
// positions split between the two waves of a SIMD; same packed weights as W36_C64_*)
#define FPC_W36P_KINDS(X) \
  X(W36P_C64_4x4, 4, 4)   \
  X(W36P_C64_2x8, 2, 8)

// W36PDKIND(name, TYT, TXT): wblock36p_dust_kernel -- the paired instance + the detector's 65th channel (same dust block)
#define FPC_W36PD_KINDS(X) \
  X(W36PD_C65_4x4, 4, 4)   \
  X(W36PD_C65_2x8, 2, 8)

// W36DKIND(name, TYT, TXT): wblock36_dust_kernel -- the 64-channel instance + the detector's 65th channel on the VALU
#define FPC_W36D_KINDS(X) \
  X(W36_C65_4x4, 4, 4)    \
  X(W36_C65_2x8, 2, 8)

// W36SKIND(name, NB, TYT, TXT): wblock36s_kernel (round 6: wblock36_kernel<NB, TYT, TXT> walking a launch's frames as one
// stacked image; chosen per LAUNCH -- w36_stacked below -- so no op of the plan carries it)
#define FPC_W36S_KINDS(X) \
  X(W36S_C128_4x4, 2, 4, 4)
// W36PCKIND(name, TYT, TXT): wconv36p_kernel (round 6: the paired body's conv-only entry point, which also admits 8 x 2)
#define FPC_W36PC_KINDS(X) \
  X(W36PC_C64_8x2, 8, 2)

enum WKind {
#define X(name, ...) WK_##name,
  FPC_WBLOCK_KINDS(X)
  FPC_W16_KINDS(X)
  FPC_W36_KINDS(X)
  FPC_W36D_KINDS(X)
  FPC_W36P_KINDS(X)
  FPC_W36PD_KINDS(X)
  FPC_W36S_KINDS(X)
  FPC_W36PC_KINDS(X)
#undef X
      WK_COUNT
};

struct WKindInfo : Instance<WBlockArgs> {
  const char* name;
  const char* symbol;
  int gen;               // 1: wblock_mfma_kernel, 2: wblock16_kernel, 3: wblock36_kernel
  int KC, NBT, CMID;
  int NCG;               // generations 2, 3: channel groups of 16
  int TH;                // tile height in pixels (8; 4 for the latency instance; generation 3: 16 or 8)
  int TW;                // tile width in pixels (16; generation 3: 16 or 32)
  bool dust = false;     // generation 3: the 65-channel (64 + dustbin) instance
};

static const WKindInfo g_wkinds[WK_COUNT] = {
#define X(name, KC, NBT, CMID)                                                                            \
  {instance_of<wblock_mfma_kernel<KC, NBT, CMID>, WBlockCfg<KC, NBT, CMID>, 512, WBlockArgs>(), #name,                         \
   "wblock_mfma_kernel<" #KC ", " #NBT ", " #CMID ">", 1, KC, NBT, CMID, 0, 8, 16},
    FPC_WBLOCK_KINDS(X)
#undef X
#define X(name, NCG, TH)                                                                                  \
  {instance_of<wblock16_kernel<NCG, TH>, W16Cfg<NCG, TH>, 512, WBlockArgs>(), #name,                                           \
   "wblock16_kernel<" #NCG ", " #TH ">", 2, 16, NCG / 2, NCG * 16, NCG, TH, 16},
    FPC_W16_KINDS(X)
#undef X
#define X(name, NB, TYT, TXT)                                                                             \
  {instance_of<wblock36_kernel<NB, TYT, TXT>, W36Cfg<NB, TYT, TXT>, 256, WBlockArgs>(), #name,                                 \
   "wblock36_kernel<" #NB ", " #TYT ", " #TXT ">", 3, 16, 2 * NB, 64 * NB, 4 * NB, 4 * TYT, 4 * TXT},
    FPC_W36_KINDS(X)
#undef X
#define X(name, TYT, TXT)                                                                                 \
  {instance_of<wblock36_dust_kernel<TYT, TXT>, W36Cfg<1, TYT, TXT, true>, 256, WBlockArgs>(), #name,                           \
   "wblock36_dust_kernel<" #TYT ", " #TXT ">", 3, 16, 2, 64, 4, 4 * TYT, 4 * TXT, true},
    FPC_W36D_KINDS(X)
#undef X
#define X(name, TYT, TXT)                                                                                 \
  {instance_of<wblock36p_kernel<TYT, TXT>, W36PCfg<TYT, TXT>, 512, WBlockArgs>(), #name,                                       \
   "wblock36p_kernel<" #TYT ", " #TXT ", 3>", 3, 16, 2, 64, 4, 4 * TYT, 4 * TXT},
    FPC_W36P_KINDS(X)
#undef X
#define X(name, TYT, TXT)                                                                                 \
  {instance_of<wblock36p_dust_kernel<TYT, TXT>, W36PCfg<TYT, TXT, true>, 512, WBlockArgs>(), #name,                            \
   "wblock36p_dust_kernel<" #TYT ", " #TXT ", 3>", 3, 16, 2, 64, 4, 4 * TYT, 4 * TXT, true},
    FPC_W36PD_KINDS(X)
#undef X
#define X(name, NB, TYT, TXT)                                                                             \
  {instance_of<wblock36s_kernel<NB, TYT, TXT>, W36Cfg<NB, TYT, TXT>, 256, WBlockArgs>(), #name,                                \
   "wblock36s_kernel<" #NB ", " #TYT ", " #TXT ">", 3, 16, 2 * NB, 64 * NB, 4 * NB, 4 * TYT, 4 * TXT},
    FPC_W36S_KINDS(X)
#undef X
#define X(name, TYT, TXT)                                                                                 \
  {instance_of<wconv36p_kernel<TYT, TXT>, W36PCfg<TYT, TXT, false, true>, 512, WBlockArgs>(), #name,                           \
   "wconv36p_kernel<" #TYT ", " #TXT ", 3>", 3, 16, 2, 64, 4, 4 * TYT, 4 * TXT},
    FPC_W36PC_KINDS(X)
#undef X
};

// ---- blob floats of every fragment layout: one function each, shared by the plan builder that reserves the region and
// the packer that fills it
// pack_conv (weights.h): `steps` K steps of 8 channels for `nbt` blocks of 32 output channels, and the two zero steps the
// kernels prefetch
static size_t conv_floats(size_t steps, int nbt) { return (steps + 2) * nbt * 64 * 4; }
// pack_conv_bf16: steps of 16 channels, `planes` terms per element
static size_t conv_bf16_floats(size_t steps, int nbt, int planes) { return (steps + 2) * planes * nbt * 64 * 4; }
static size_t bias_floats(int nbt) { return (size_t)nbt * 32; }
// a Winograd kernel's conv1 fragments.  Generations 2, 3: [channel group][chunk of 16][position][64 lanes] float4 + zero
// positions behind every group (the fragment rings read ahead); generation 1: pack_conv's order with 16 positions for
// taps, and a chunk of zeros
static size_t w1_floats(const WKindInfo& k, int nchunk) {
  if (k.gen == 3) return (size_t)k.NCG * ((size_t)nchunk * 36 + (k.NCG == 8 ? W36Cfg<2, 4, 4>::WPAD : W36Cfg<1, 4, 4>::WPAD)) * 256;
  if (k.gen == 2) return (size_t)k.NCG * ((size_t)nchunk * 16 + W16Cfg<8>::WPAD) * 256;
  return conv_floats(((size_t)nchunk + 1) * 16 * (k.KC / 8), k.NBT);
}
// ... and its 1x1 stage's, over `k8` steps of 8 channels of [h | x]: [channel group][step of 16][lane] float4 (pack_w16_1x1),
// generation 1: pack_conv's
static size_t w2_floats(const WKindInfo& k, int k8) {
  if (k.gen >= 2) return (size_t)k.NCG * ((size_t)k8 / 2 + W16Cfg<8>::WPAD) * 256;
  return conv_floats(k8, k.NBT);
}
// MFMA FLOPs one frame's tiles issue: positions x Winograd tiles x channels x K for the 3x3, pixels x channels x K for the 1x1
static double wkind_mfma_flops(const WKindInfo& k, int tiles, int nchunk, int k8_1x1) {
  const double px = (double)k.TH * k.TW, n = k.NBT * 32.0;
  if (k.gen == 3) return 2.0 * tiles * n * (36.0 * (px / 16) * nchunk * k.KC + px * k8_1x1 * 8.0);
  return 2.0 * tiles * n * (16.0 * (px / 4) * nchunk * k.KC + px * k8_1x1 * 8.0);
}
// Generation 3 addresses its tensors with signed 32-bit byte offsets below W36_MARKER (wblock36_mfma.h).  A launch is
// given pointers to ITS first frame (round 4; round 3 addressed from the batch's frame 0 and sent a layer whose whole
// tensor did not fit -- the C++ network's full-resolution layers at 32 frames -- to generation 2) and is split into
// several launches where even its own frames do not fit; only a layer whose single frame is too large falls back.
static bool w36_fits(int /*B*/, int H, int W, int cs_in, int cs_out) {
  return (unsigned long long)H * W * (unsigned long long)std::max(cs_in, cs_out) * sizeof(float) < (unsigned long long)W36_MARKER;
}
static int w36_frames_per_launch(int H, int W, int cs_in, int cs_out) {
  const unsigned long long fb = (unsigned long long)H * W * (unsigned long long)std::max(cs_in, cs_out) * sizeof(float);
  return (int)std::max<unsigned long long>(1, ((unsigned long long)W36_MARKER - 1) / fb);
}
// Generation 2 (wblock16_kernel) reads its input through ONE buffer descriptor that starts at the tensor's frame 0, with
// unsigned 32-bit byte offsets (wblock16_mfma.h: load_halo; launch_wblock clamps the descriptor's range to W16_REACH): a
// frame that ends beyond W16_REACH bytes would read zeros or, past 2^32, the pixels of an earlier frame.  The Python
// network's widest generation-2 input has 16 bytes per frame pixel, which fpc_create's 2^28-pixel limit keeps in reach;
// the C++ network's full-resolution layers have 256.  The frames of an H x W tensor with `cs` channels that are in reach:
static const unsigned long long W16_REACH = 0xfffffff0ull;
static int w16_frames_in_reach(int H, int W, int cs) {
  return (int)std::min<unsigned long long>(1u << 30, W16_REACH / ((unsigned long long)H * W * cs * sizeof(float)));
}
// conv-only layers wider than one instance: two 128-channel parts or four 64-channel ones (NB = 1 tiles take 0.53 of an
// NB = 2 tile's time) -- whichever needs fewer tile times on `cus` CUs for `tiles` tiles per part
static int w36_conv_part(int cout, int tiles, int cus) {
  if (cout < 128) return 64;
  if (cout == 128) return 128;
  const double t2 = std::ceil((double)tiles * (cout / 128) / cus) * 1.0, t1 = std::ceil((double)tiles * (cout / 64) / cus) * 0.53;
  return t1 < t2 ? 64 : 128;
}
// Generation 3: the arrangement of the 16 Winograd tiles (4 x 4 or 2 x 8) that covers the map with fewer tiles
// (cout == 64, `paired`: the two-waves-per-SIMD instance, wblock36p_mfma.h -- the default since round 5; a block's
// projection must then be a multiple of 64 channels wide, which every 64-channel layer of both networks is)
// (`conv82`, round 6: a conv-only 64-channel paired launch may also take 8 x 2 -- 32 x 8 pixels, wconv36p_kernel -- where
// that needs fewer tiles than both: a 30 x 40 map is 5 of them against 6 and 8.  A tie keeps the choice without it.)
static WKind w36_kind(int cout, int H, int W, bool paired = false, bool conv82 = false) {
  const int t44 = ((H + 15) / 16) * ((W + 15) / 16), t28 = ((H + 7) / 8) * ((W + 31) / 32), t82 = ((H + 31) / 32) * ((W + 7) / 8);
  if (conv82 && cout == 64 && paired && t82 < std::min(t44, t28)) return WK_W36PC_C64_8x2;
  if (cout == 65 && paired) return t28 < t44 ? WK_W36PD_C65_2x8 : WK_W36PD_C65_4x4;
  if (cout == 65) return t28 < t44 ? WK_W36_C65_2x8 : WK_W36_C65_4x4;
  if (cout == 64 && paired) return t28 < t44 ? WK_W36P_C64_2x8 : WK_W36P_C64_4x4;
  if (cout == 64) return t28 < t44 ? WK_W36_C64_2x8 : WK_W36_C64_4x4;
  return t28 < t44 ? WK_W36_C128_2x8 : WK_W36_C128_4x4;
}

// Round 6: the instance that walks a launch's frames as one stacked image for an op on `wk` (WK_COUNT: none).  The 128-channel
// arrangements share their fragments, so a 2 x 8 op may take the 4 x 4 stacked walk too.
static WKind w36_stacked_kind(WKind wk) { return wk == WK_W36_C128_4x4 || wk == WK_W36_C128_2x8 ? WK_W36S_C128_4x4 : WK_COUNT; }
// ... and its tile rows for `frames` frames of Hf x W on instance `sk`, where that is FEWER tiles than the `tiles_now` per
// frame the op launches frame by frame (60 rows on 16-row tiles: 18.75 tile rows per frame instead of 20; a height that is
// a multiple of the tile's gains nothing) -- 0 where it is not, or where the kernel does not apply: it needs every
// Winograd tile inside one frame (Hf % 4 == 0) and at most one seam per tile (Hf >= the tile's height).
static int w36_stacked_rows(int Hf, int W, int frames, WKind sk, int tiles_now) {
  if (sk == WK_COUNT) return 0;
  const int th = g_wkinds[sk].TH, tw = g_wkinds[sk].TW;
  if (Hf % 4 != 0 || Hf < th) return 0;
  const int rows = (frames * Hf + th - 1) / th;
  return rows * ((W + tw - 1) / tw) < frames * tiles_now ? rows : 0;
}

// bf16 / split-operand instances.  FKIND(name, KERNEL, CFG, PLANES, TH,TW, S,EXT, KC, WM,WN, MB,NB, CMIDP)
//   PLANES 1: block_bf16_kernel (dtype = FPC_BF16); 3: block_x3_kernel (dtype = FPC_F32_SPLIT)
#define FPC_BF16_KINDS(X)                                                                   \
  X(F816_s1_K64_C64, block_bf16_one_kernel, BlockBfCfg, 1, 8, 32, 1, 3, 64, 2, 2, 4, 1, 64) \
  X(F816_s1_K64_C128, block_bf16_kernel, BlockBfCfg, 1, 8, 16, 1, 3, 64, 1, 4, 4, 1, 128)   \
  X(F816_s1_K80_C80, block_bf16_one_kernel, BlockBfCfg, 1, 8, 16, 1, 3, 80, 4, 1, 1, 3, 80) \
  X(F816_s1_K128_C128, block_bf16_one_kernel, BlockBfCfg, 1, 8, 16, 1, 3, 128, 1, 4, 4, 1, 128) \
  X(F816_s1_K128_C80w, block_bf16_one_kernel, BlockBfCfg, 1, 8, 16, 1, 3, 128, 1, 4, 4, 1, 80) \
  X(F620_s2_K64_C128, block_bf16_one_kernel, BlockBfCfg, 1, 6, 20, 2, 3, 64, 2, 2, 2, 2, 128) \
  X(F320_s2_K128_C256, block_bf16_one_kernel, BlockBfCfg, 1, 3, 20, 2, 3, 128, 1, 4, 2, 2, 256) \
  X(F416_s1_K128_C256, block_bf16_two_kernel, BlockBfCfg, 1, 4, 16, 1, 3, 128, 1, 4, 2, 2, 256) \
  X(F816_ct_K64_C128, block_bf16_kernel, BlockBfCfg, 1, 8, 16, 1, 2, 64, 1, 4, 4, 1, 128)   \
  X(F816_ctf_K64_C128, convt_bf16_kernel, ConvTBfCfg, 1, 8, 16, 1, 2, 64, 2, 2, 2, 1, 128)  \
  X(S816_s1_K64_C64, block_x3_kernel, BlockX3Cfg, 3, 8, 16, 1, 3, 64, 2, 2, 2, 1, 64)       \
  X(S620_s2_K16_C128, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 2, 3, 16, 2, 2, 2, 2, 128)     \
  X(S620_s1_K64_C128, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 1, 3, 64, 2, 2, 2, 2, 128)     \
  X(S620_s1_K64_C80, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 1, 3, 64, 4, 1, 1, 3, 80)       \
  X(S620_s1_K16_C80, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 1, 3, 16, 4, 1, 1, 3, 80)       \
  X(S320_s2_K16_C256, block_x3_kernel, BlockX3Cfg, 3, 3, 20, 2, 3, 16, 1, 4, 2, 2, 256)     \
  X(S320_s1_K64_C256, block_x3_kernel, BlockX3Cfg, 3, 3, 20, 1, 3, 64, 1, 4, 2, 2, 256)     \
  X(S620_ct_K64_C128, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 1, 2, 64, 2, 2, 2, 2, 128)     \
  X(S620_1x1_K64_C80, block_x3_kernel, BlockX3Cfg, 3, 6, 20, 1, 1, 64, 4, 1, 1, 3, 80)      \
  X(S320_1x1_K64_C256, block_x3_kernel, BlockX3Cfg, 3, 3, 20, 1, 1, 64, 1, 4, 2, 2, 256)     \
  X(H816_s1_K64_C64, block_h2_kernel, BlockH2Cfg, 2, 8, 16, 1, 3, 64, 2, 2, 2, 1, 64)     \
  X(H620_s2_K16_C128, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 2, 3, 16, 2, 2, 2, 2, 128)     \
  X(H620_s1_K64_C128, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 1, 3, 64, 2, 2, 2, 2, 128)     \
  X(H620_s1_K64_C80, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 1, 3, 64, 4, 1, 1, 3, 80)     \
  X(H620_s1_K16_C80, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 1, 3, 16, 4, 1, 1, 3, 80)     \
  X(H320_s2_K16_C256, block_h2_kernel, BlockH2Cfg, 2, 3, 20, 2, 3, 16, 1, 4, 2, 2, 256)     \
  X(H320_s1_K64_C256, block_h2_kernel, BlockH2Cfg, 2, 3, 20, 1, 3, 64, 1, 4, 2, 2, 256)     \
  X(H620_ct_K64_C128, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 1, 2, 64, 2, 2, 2, 2, 128)     \
  X(H620_1x1_K64_C80, block_h2_kernel, BlockH2Cfg, 2, 6, 20, 1, 1, 64, 4, 1, 1, 3, 80)     \
  X(H320_1x1_K64_C256, block_h2_kernel, BlockH2Cfg, 2, 3, 20, 1, 1, 64, 1, 4, 2, 2, 256)

enum FKind {
#define X(name, ...) FK_##name,
  FPC_BF16_KINDS(X)
#undef X
      FK_COUNT
};

struct FKindInfo : Instance<BlockBfArgs> {
  const char* name;
  const char* symbol;
  int planes, TH, TW, S, EXT, KC, WM, WN, MB, NB, CMIDP;
};

static const FKindInfo g_fkinds[FK_COUNT] = {
#define X(name, KERN, CFG, PL, TH, TW, S, EXT, KC, WM, WN, MB, NB, CMIDP)                                                                  \
  {instance_of<KERN<TH, TW, S, EXT, KC, WM, WN, MB, NB, CMIDP>, CFG<TH, TW, S, EXT, KC, WM, WN, MB, NB, CMIDP>, WM * WN * 64, BlockBfArgs>(), \
   #name, #KERN "<" #TH ", " #TW ", " #S ", " #EXT ", " #KC ", " #WM ", " #WN ", " #MB ", " #NB ", " #CMIDP ">",                             \
   PL, TH, TW, S, EXT, KC, WM, WN, MB, NB, CMIDP},
    FPC_BF16_KINDS(X)
#undef X
};

// What prepare_kernels does with a table: the dynamic-LDS limit of every instance; under FPC_DIAG, its occupancy
template <typename Info, size_t N>
static int allow_dynamic_lds(const Info (&table)[N]) {
  for (const Info& k : table) HIPCHECK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes));
  return FPC_OK;
}
#ifdef FPC_DIAG
template <typename Info, size_t N>
static void print_occupancy(const Info (&table)[N]) {
  for (const Info& k : table) {
    int nb = -1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, k.threads, k.lds_bytes);
    hipFuncAttributes fa{};
    hipFuncGetAttributes(&fa, k.fn);
    fprintf(stderr, "[diag] %s: lds %d B, regs %d, scratch %zu, static lds %zu, occupancy %d blocks/CU\n", k.name, k.lds_bytes,
            fa.numRegs, fa.localSizeBytes, fa.sharedSizeBytes, nb);
  }
}
#endif

// ------------------------------------------------------------------------------------
// Launch plan
// ------------------------------------------------------------------------------------
enum OpType { OP_STEM, OP_POOL, OP_CONV, OP_BLOCK, OP_WBLOCK, OP_BF16, OP_SOFTMAX, OP_NMS, OP_DESC,
              OP_VCONV0, OP_POOL2, OP_L2NORM };

struct Op {
  OpType type;
  std::string name;
  Kind kind = K_COUNT;
  ConvArgs args{};
  BKind bkind = BK_COUNT;
  BlockArgs bargs{};
  WKind wkind = WK_COUNT;
  int hash_bkind = -1, hash_wkind = -1;   // round 6: the instance FPC_PLAN_TILES_ROUND5 launches where `bkind` / `wkind` is a re-tiling of it (same fragments): what plan_hash mixes, so blobs travel between the two plans
  WBlockArgs wargs{};
  FKind fkind = FK_COUNT;
  BlockBfArgs fargs{};
  int phase = -1;              // ConvTranspose output-parity phase of a bf16 conv-only op
  int when = 0;                // 0: always; 1: only in calls of a few frames; 2: only in larger calls
  bool shadow = false;         // packed like any op but never launched: part 1 .. G - 1 of a conv-only launch of G parts (add_wconv merges them into part 0's op)
  bool wconv = false;          // conv-only Winograd launch: 3x3 conv + (BN or bias) + ReLU, output channels n0 .. n0+127
  int n0 = 0;
  bool plain_conv = false;     // a Conv2d + bias (+ ReLU) of the C++ network: weights `prefix`.weight / .bias, no BN
  bool lean = false;           // OP_CONV on conv2_mfma_kernel (round 5; add_conv decides)
  int ksize = 0;
  const float* pin = nullptr;  // OP_POOL2 / OP_L2NORM / OP_VCONV0 operands
  float* pout = nullptr;
  int pH = 0, pW = 0, pC = 0;
  std::string prefix;          // checkpoint prefix of a fused block
  int cin = 0, cout = 0;       // real channel counts of a fused block
  int grid_y = 1, grid_z = 1;
  double flops_per_frame = 0;  // algorithmic: 2 * MACs of the real (unpadded) convolution
  double mfma_flops_per_frame = 0;  // issued on the matrix cores (padding included; Winograd: 16/36 of the 3x3)
  bool fused_softmax_capable = false;   // FPC_BF16's detector.layer.1 (block_bf16.h: fused exp-softmax epilogue)
  double bytes_per_frame = 0;       // algorithmic HBM bytes: the launch's input tensor(s) read once + its output written once
  bool descriptor_branch = false;
};

// `len` floats of the packed blob from float `off`: what a plan builder reserved for one fragment or bias vector (reserve);
// the packers write no more into it (Packer).  plan_hash mixes the offsets alone.
struct Region {
  size_t off = 0, len = 0;
};

struct Timing {
  hipEvent_t start, stop;
  int op;
  int frames;  // frames covered by this launch (a sub-batch)
  int wkind = -1;            // round 6: the instance that ran where it is not the op's (the stacked walk) ...
  double mfma_flops = -1.0;  // ... and what its tiles issued
};

// One device allocation of a context: carved by a Carver, zeroed, its canary zones (offset, bytes) filled where the
// context has them.  A context owns eight (fpc_ctx::slabs).
using GuardZones = std::vector<std::pair<size_t, size_t>>;
struct Carver;
struct Slab {
  char* base = nullptr;
  size_t bytes = 0;
  GuardZones zones;
  explicit operator bool() const { return base != nullptr; }
  int allocate(hipStream_t st, Carver& cv);
  hipError_t release() {
    const hipError_t e = base ? hipFree(base) : hipSuccess;
    *this = Slab{};
    return e;
  }
};

}  // namespace fpc

using namespace fpc;

struct fpc_ctx {
  fpc_config cfg{};
  int H = 0, W = 0, B = 0, Hc = 0, Wc = 0;
  bool vgg = false;                  // cfg.arch == FPC_ARCH_VGG: superpoint::SPModel (cpp/src/model.cc)
  int D = 128;                       // descriptor length: 128 (python net) / 256 (C++ net, settings.h:25)
  struct VTap { const char* name; const float* p; int cs, C, H, W; };   // a tensor of the C++ network: buffer, channel stride, shape
  std::vector<VTap> vtaps;           // ... by the reference's module names (build_vgg_plan; fpc_read_activation)
  size_t vconv0_off = 0;
  bool bf16 = false;                 // cfg.dtype == FPC_BF16
  bool split = false;                // cfg.dtype == FPC_F32_SPLIT or FPC_F32_SPLIT_F16
  bool split_f16 = false;            // ... the latter: two fp16 terms per operand, three MFMAs per product
  int lgcs = 72;                     // channel stride of the logits buffer (80 in bf16 mode)
  int cin = 3;                       // 3: [n,3,H,W] frames (the reference's layout); 1: gray [n,1,H,W]
  int cap = 0, sort_cap = 0;
  PlanOptions opt;                   // plan_options.h: every launch-plan option, resolved once by fpc_create
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t upload = nullptr;       // fpc_upload_stream: the caller's copy stream, on a hardware queue of its own
  bool queue_probe = true;            // fpc_create placed the streams on hardware queues of their own (queue_map.h; FPC_QUEUE_PROBE)
  int probe_rounds = 0;               // ... with this many probe rounds, in this much host time (fpc_stream_report)
  double placement_ms = 0.0;
  std::vector<std::pair<hipStream_t, int>> caller_stream_memo;   // fpc_set_stream: queue classes of the caller's streams seen before (at most 4)
  std::vector<hipStream_t> aux;      // extra streams for sub-batches
  std::vector<hipEvent_t> ev_join;
  std::vector<hipStream_t> side;     // per sub-batch: detector head + NMS next to the descriptor head
  std::vector<hipEvent_t> ev_enc, ev_det;
  hipEvent_t ev_fork = nullptr;
  int small_reach = 1 << 30;         // the C++ network: the largest call the latency plan's generation-2 launches can address (build_vgg_plan)
  int num_cus = 256;
  int fkind_blocks_per_cu[64] = {};   // resident workgroups per CU of every bf16 / split-operand instance (fpc_create)
  bool logits_valid = false;       // the last call wrote the logits ("det.1" of fpc_read_activation): false after a fused-softmax fpc_detect
#ifdef FPC_DIAG
  unsigned long long* diag_stamps = nullptr;
  int diag_n = 0;
#endif
  bool weights_loaded = false;
  bool plan_error = false;           // a layer asked for a kernel instance that does not exist (fpc_create -> FPC_E_INVALID)

  // The eight device allocations a context can own: `slab` for all activations / results (build_plan), the others made
  // by the call that reserves them.  bank_slab, topk_slab, pnp_topk_slab and lm_slab go with the bank; fpc_destroy frees
  // what is left.
  Slab slab, bank_slab, topk_slab, pnp_slab, lm_slab, pnp_topk_slab, window_slab, graph_slab;
  Slab* const slabs[8] = {&slab, &bank_slab, &topk_slab, &pnp_slab, &lm_slab, &pnp_topk_slab, &window_slab, &graph_slab};
  float *stem_out, *x0, *h4, *x1, *x2, *h8, *x3, *cat, *dh, *dproj, *d0, *lg;
  float *h16, *y16a, *y16b, *lo_h, *lo0, *desc_map, *desc_in_nhwc;
  float* prob;
  uint32_t *nmsmap, *cand;
  int32_t *ncand, *count, *xy, *status;
  float* rowmax = nullptr;          // [B][H / 8]: the largest logit of every row of cells of the last call
  uint32_t* range = nullptr;        // [B][FPC_RANGE_WORDS]: largest logit / descriptor-map value, non-finite input flag, per frame
  float *conf, *desc_out;
  unsigned long long* sort_scratch;
  int32_t* nms_aux = nullptr;  // [B][NMS_AUX_INTS] (kernels_misc.h: nms_chunk_sort_kernel)
  unsigned long long *rowbest, *colbest;  // descriptor matching workspace, `cap` entries each
  // batched matching (fpc_match_frames / fpc_first_within_frames): norms [(B + 1)][cap], top-2 [B][cap][2],
  // column minima [B][cap] -- carved behind the buffers above (null where descriptors are off)
  float* mf_norms = nullptr;
  unsigned long long *mf_top2 = nullptr, *mf_colbest = nullptr;
  // RANSAC homographies (fpc_ransac_homography / fpc_homography_frames): pair lists [B][cap] of 16-byte records, the mask
  // row of every pair [B][cap], pair counts [B], best keys [B] -- carved with or without descriptors
  float4* hf_pairs = nullptr;
  int32_t *hf_row = nullptr, *hf_np = nullptr;
  unsigned long long* hf_best = nullptr;
  // cell-ordered guided matching (fpc_match_*_guided_cells, match_guided_cells.h): the orders of the query sets and of the
  // train sets [B][cap] each, the boxes of their runs of 64 ordered rows [2][B][ceil(cap / 64)] -- behind the RANSAC buffers
  int32_t *mgc_perm_q = nullptr, *mgc_perm_t = nullptr;
  int4* mgc_box = nullptr;
  // key-frame bank (fpc_bank_*, fpc_match_bank, fpc_homography_bank): one allocation of its own, made by fpc_bank_create --
  // storage, per-slot norms and fpc_match_bank's workspace, carved with canary zones in a FPC_PLAN_GUARD_ZONES context
  BankArgs bank{};
  int bank_format = FPC_BANK_F32;                              // FPC_BANK_BF16: bank.desc is null, the rows are bank16.desc
  BankBf16Args bank16{};                                       // (match_bank_bf16.h)
  // top-K candidates of the bank (fpc_bank_topk_reserve, match_bank_topk.h): a third allocation, made by that call and
  // freed with the bank -- the pair tables of max_batch x kmax (frame, candidate) pairs and the RANSAC workspace (pair
  // lists, rows, counts, best keys) of as many problems
  BankTopkArgs topk{};
  float4* topk_pairs = nullptr;
  int32_t *topk_row = nullptr, *topk_np = nullptr;
  unsigned long long* topk_best = nullptr;
  // RANSAC PnP (fpc_pnp_reserve, pnp_ransac.h): an allocation of its own, made by that call and freed by fpc_destroy -- the
  // pair records (with their mask rows), counts and best keys of max_batch problems
  float4* pnp_rec = nullptr;
  int32_t* pnp_np = nullptr;
  unsigned long long* pnp_best = nullptr;
  // absolute pose per top-K candidate (fpc_pnp_topk_reserve): the same three buffers for max_batch x kmax problems, an
  // allocation of its own, made by that call and freed with the bank
  float4* pnp_topk_rec = nullptr;
  int32_t* pnp_topk_np = nullptr;
  unsigned long long* pnp_topk_best = nullptr;
  // landmarks of the bank's rows (fpc_bank_landmarks_reserve): float4 [slots][rows], w = 1 valid / 0; freed with the bank
  float4* lm_xyzw = nullptr;
  // local bundle adjustment (fpc_window_reserve, refine_window.h): an allocation of its own, freed by fpc_destroy -- the
  // observation table and pixels [16][cap], the key pixels, flags and stepped points [cap], the chunks' partial sums and
  // the pose state
  RwArgs rw{};
  // pose graph (fpc_graph_reserve, pose_graph.h): an allocation of its own, freed by fpc_destroy -- the nodes, the edges and
  // their counters, the stepped state, the adjacency, the linearisation and the solve's vectors
  PgArgs pg{};
  int pts_n = 0;                     // frames of the last call that produced keypoints (fpc_detect*, fpc_get_points)
  bool pts_desc = false;             // ... and whether it sampled their descriptors

  float* u8stage = nullptr;          // fpc_detect_u8: converted frames [B,cin,H,W], allocated on first use
  char* ha_ws = nullptr;             // fpc_homography_adaptation: workspace, allocated on first use

  // packed weights
  float* blob = nullptr;
  size_t blob_floats = 0;
  uint32_t* bcast_tag = nullptr;   // 64 bytes of the slab: fpc_broadcast_weights' first collective (allocated here so that it cannot fail there)
  std::vector<float> host_blob;

  std::vector<Op> ops;
  StemArgs stem{};
  size_t stem_w_off = 0, stem_b_off = 0;
  struct ConvW {
    Region w[4], b, b2;   // fragments (OP_CONV: one per grid z; blocks: conv1, the 1x1 stage, the dust block), biases
  };
  std::vector<ConvW> convw;  // parallel to ops (unused entries for non-conv ops)

  bool timing = false;               // this call is timed (LaunchTimer)
  int timing_every = 0, timing_calls = 0;   // fpc_set_timing(n): one fpc_detect call in n is timed (0 = off)
  std::vector<Timing> timings;
  std::vector<hipEvent_t> event_pool;
  size_t events_used = 0;
};

namespace fpc {

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// FPC_PLAN_GUARD_ZONES (a test facility, include/fpc.h): `guard` bytes of a canary pattern behind EVERY carved buffer and
// GUARD_TAIL bytes behind the last one -- the out-of-range store this exists for ("a fault worth
// recording") landed W36_MARKER = 2 GiB behind its tensor, so the tail zone spans that distance from any buffer of a
// small configuration.  fpc_check_guards counts the words that no longer hold the pattern.
constexpr size_t GUARD_BYTES = 64 << 10;
constexpr size_t GUARD_TAIL = (size_t)0x80000000u + (4u << 20);
constexpr uint32_t GUARD_PATTERN = 0xA5C3F00Du;

struct Carver {
  size_t off = 0;
  size_t guard = 0;
  GuardZones zones;   // (offset, bytes) of every guard zone
  // a carver for one of `c`'s slabs: zones behind its buffers where the context has them
  explicit Carver(const fpc_ctx* c) : guard(c->opt.guard_zones ? GUARD_BYTES : 0) {}
  template <typename T>
  size_t take(size_t n) {
    const size_t o = off;
    off = align_up(off + n * sizeof(T), 256);
    if (guard) {
      zones.push_back({off, guard});
      off += guard;
    }
    return o;
  }
  // take<T>(n) for a buffer whose pointer `*slot` becomes once the slab exists (bind): taken and assigned in one place
  struct Bound { void* slot; size_t off; };
  std::vector<Bound> bound;
  template <typename T>
  void into(T** slot, size_t n) { bound.push_back({slot, take<T>(n)}); }
  void bind(char* slab) const {
    for (const Bound& b : bound) {
      char* p = slab + b.off;
      memcpy(b.slot, &p, sizeof p);
    }
  }
  void finish() {
    if (guard) {
      zones.push_back({off, GUARD_TAIL});
      off += GUARD_TAIL;
    }
  }
};

__global__ void guard_fill_kernel(uint32_t* p, size_t n, uint32_t v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void guard_count_kernel(const uint32_t* p, size_t n, uint32_t v, unsigned long long* bad) {
  unsigned long long mine = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) mine += p[i] != v;
  if (mine) atomicAdd(bad, mine);
}
static unsigned guard_blocks(size_t words) { return (unsigned)std::min<size_t>(4096, (words + 255) / 256); }

// One slab's zones on stream `st`: written, or their damaged words counted.
static void fill_zones(hipStream_t st, char* base, const GuardZones& zones) {
  for (const auto& z : zones) {
    const size_t n = z.second / 4;
    guard_fill_kernel<<<guard_blocks(n), 256, 0, st>>>(reinterpret_cast<uint32_t*>(base + z.first), n, GUARD_PATTERN);
  }
}
static void count_zones(hipStream_t st, const Slab& s, unsigned long long* bad) {
  for (const auto& z : s.zones) {
    const size_t n = z.second / 4;
    guard_count_kernel<<<guard_blocks(n), 256, 0, st>>>(reinterpret_cast<const uint32_t*>(s.base + z.first), n, GUARD_PATTERN, bad);
  }
}

static int fill_guards(fpc_ctx* c) {
  // (the hipMemset of the workspace in front of this call runs on the null stream and need not have finished when it
  // returns; c->stream is non-blocking, so nothing orders the two -- the first version lost 2 MB of pattern to it.
  // Waited for in every context: the first call's kernels must not race the zeroing either.)
  HIPCHECK(hipDeviceSynchronize());
  fill_zones(c->stream, c->slab.base, c->slab.zones);
  if (!c->slab.zones.empty()) HIPCHECK(hipStreamSynchronize(c->stream));
  return FPC_OK;
}

// The cv.off bytes a finished carver asks for: zeroed, then the zones the carver listed filled on `st` -- behind a device
// synchronise, as in fill_guards: the null stream's memset does not order `st`.  Then every pointer taken with
// Carver::into is assigned.  On failure nothing stays allocated, and neither the slab nor those pointers are touched.
int Slab::allocate(hipStream_t st, Carver& cv) {
  char* p = nullptr;
  HIPCHECK(hipMalloc((void**)&p, cv.off));
  hipError_t e = hipMemset(p, 0, cv.off);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  fill_zones(st, p, cv.zones);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) hipFree(p);
  HIPCHECK(e);
  base = p;
  bytes = cv.off;
  zones = std::move(cv.zones);
  cv.bind(p);
  return FPC_OK;
}

// ---- architecture walk ---------------------------------------------------------------
// Builds ctx->ops with geometry and buffer pointers, and assigns blob offsets.  The
// weight VALUES are filled by pack_all() when a checkpoint arrives.

// The rest of the slab behind a network's activations: what post-processing, matching, RANSAC and the cell orders use,
// the same buffers in the same order for both networks.  Then the slab itself: allocated, zeroed, its canary zones
// filled, every pointer taken with Carver::into assigned.
static int carve_results(fpc_ctx* c, Carver& cv) {
  const size_t B = c->B, HW = (size_t)c->H * c->W, cap = c->cap;
  // the matching buffers shrink to a stub where the Python network runs without descriptors (the C++ network's plan
  // has always carved them whole)
  const bool whole = c->vgg || c->cfg.descriptor_enabled != 0;
  cv.into(&c->prob, B * HW);
  cv.into(&c->nmsmap, B * HW); cv.into(&c->cand, B * HW);
  cv.into(&c->ncand, B); cv.into(&c->count, B);
  cv.into(&c->status, 4 + BLOB_HEADER_FLOATS);   // + the 64-byte tag of fpc_broadcast_weights
  cv.into(&c->range, B * FPC_RANGE_WORDS);       // per-frame range words (kernels_misc.h)
  cv.into(&c->rowmax, B * (c->H / 8));           // largest logit per row of cells (softmax_d2s_kernel)
  cv.into(&c->xy, B * cap * 2); cv.into(&c->conf, B * cap);
  cv.into(&c->desc_out, whole ? B * cap * c->D : 64);
  cv.into(&c->sort_scratch, B * c->sort_cap);
  cv.into(&c->nms_aux, B * NMS_AUX_INTS);
  cv.into(&c->rowbest, cap); cv.into(&c->colbest, cap);
  cv.into(&c->mf_norms, whole ? (B + 1) * cap : 64);
  cv.into(&c->mf_top2, whole ? B * cap * 2 : 64);
  cv.into(&c->mf_colbest, whole ? B * cap : 64);
  cv.into(&c->hf_pairs, B * cap); cv.into(&c->hf_row, B * cap);
  cv.into(&c->hf_np, B); cv.into(&c->hf_best, B);
  cv.into(&c->mgc_perm_q, whole ? B * cap : 64); cv.into(&c->mgc_perm_t, whole ? B * cap : 64);
  cv.into(&c->mgc_box, whole ? 2 * B * ((cap + 63) / 64) : 64);
  cv.finish();
  c->slab.bytes = cv.off;
  c->slab.zones = cv.zones;
  if (hipMalloc((void**)&c->slab.base, c->slab.bytes) != hipSuccess) {
    g_hip_err = "hipMalloc(workspace " + std::to_string(c->slab.bytes >> 20) + " MiB) failed";
    return FPC_E_HIP;
  }
  HIPCHECK(hipMemset(c->slab.base, 0, c->slab.bytes));
  if (int grc = fill_guards(c)) return grc;
  cv.bind(c->slab.base);
  c->bcast_tag = reinterpret_cast<uint32_t*>(c->status + 4);
  return FPC_OK;
}

// An op without weights of its own: its (unused) blob offsets keep `convw` parallel to `ops`
static Op& push_op(fpc_ctx* c, OpType type, const std::string& name) {
  Op op;
  op.type = type;
  op.name = name;
  c->ops.push_back(op);
  c->convw.push_back({});
  return c->ops.back();
}

// The end of either network's plan: the post-processing ops, the blob, and every op's weight pointers into it.
// (A conv-only Winograd or split-operand op has no second stage: its w[1] and b2 are empty at offset 0, so w2 / b2 point at the
// blob's tag, in bounds, and the kernels do not read them under conv_only.)
static int finish_plan(fpc_ctx* c, size_t blob_floats) {
  push_op(c, OP_NMS, "nms+sort+border_crop");
  if (c->cfg.descriptor_enabled) push_op(c, OP_DESC, "descriptor_sample+l2norm");
  for (Op& op : c->ops)
    if (op.type == OP_SOFTMAX) op.bytes_per_frame = 4.0 * (65.0 * c->Hc * c->Wc + 2.0 * c->H * c->W);   // logits in; prob + NMS state map out
  c->blob_floats = blob_floats;
  HIPCHECK(hipMalloc((void**)&c->blob, c->blob_floats * sizeof(float)));
  HIPCHECK(hipMemset(c->blob, 0, c->blob_floats * sizeof(float)));
  for (size_t i = 0; i < c->ops.size(); ++i) {
    Op& op = c->ops[i];
    const fpc_ctx::ConvW& cw = c->convw[i];
    const float *w1 = c->blob + cw.w[0].off, *w2 = c->blob + cw.w[1].off, *b1 = c->blob + cw.b.off, *b2 = c->blob + cw.b2.off;
    switch (op.type) {
      case OP_WBLOCK:
        op.wargs.w1 = reinterpret_cast<const float4*>(w1); op.wargs.b1 = b1;
        op.wargs.w2 = reinterpret_cast<const float4*>(w2); op.wargs.b2 = b2;
        op.wargs.dust = g_wkinds[op.wkind].dust ? c->blob + cw.w[2].off : nullptr;
        break;
      case OP_BF16:
        op.fargs.w1 = reinterpret_cast<const uint4*>(w1); op.fargs.b1 = b1;
        op.fargs.w2 = reinterpret_cast<const uint4*>(w2); op.fargs.b2 = b2;
        break;
      case OP_BLOCK:
        op.bargs.w1 = reinterpret_cast<const float4*>(w1); op.bargs.b1 = b1;
        op.bargs.w2 = reinterpret_cast<const float4*>(w2); op.bargs.b2 = b2;
        break;
      case OP_CONV:
        for (int z = 0; z < op.grid_z; ++z)
          op.args.sub[z].wfrag = reinterpret_cast<const float4*>(c->blob + cw.w[z].off);
        op.args.bias = b1;
        break;
      default:
        break;
    }
  }
  return FPC_OK;
}

// The next `n` floats of the blob become region `r`
static void reserve(size_t* blob_off, Region& r, size_t n) {
  r = {*blob_off, n};
  *blob_off += n;
}
// An op with weights: what the packers and the reports read of it, whichever kernel family runs it
static Op weight_op(OpType type, const std::string& name, const std::string& prefix, int cin, int cout, bool desc_branch) {
  Op op;
  op.type = type; op.name = name; op.prefix = prefix;
  op.cin = cin; op.cout = cout; op.descriptor_branch = desc_branch;
  return op;
}
static void push_op(fpc_ctx* c, const Op& op, const fpc_ctx::ConvW& cw) {
  c->ops.push_back(op);
  c->convw.push_back(cw);
}
// A layer's two variants: the ops from `i0` on run only in calls of a few frames (when = 1) or only in larger calls (2)
static void mark_when(fpc_ctx* c, size_t i0, int when) {
  for (size_t k = i0; k < c->ops.size(); ++k) c->ops[k].when = when;
}
static unsigned x_bytes(const fpc_ctx* c, int H, int W, int csx, int elem) {
  return (unsigned)std::min<size_t>((size_t)c->B * H * W * csx * elem, 0xffffff00u);
}

// ConvTranspose2d(k3, s2, p1, op1) as four output-parity phases over the INPUT grid: the taps of phase `ph` = 2 py + px in
// the order the plan lays them out and the packers fill them -- input pixel (dy, dx) of the halo under weight (ky, kx)
struct ConvTTap { int dy, dx, ky, kx; };
static std::vector<ConvTTap> convt_phase_taps(int ph) {
  const int py = ph >> 1, px = ph & 1;
  std::vector<ConvTTap> taps;
  for (int iy = 0; iy < (py ? 2 : 1); ++iy)
    for (int ix = 0; ix < (px ? 2 : 1); ++ix)   // py=1: (dy=1,ky=0), (dy=0,ky=2)
      taps.push_back({py ? 1 - iy : 0, px ? 1 - ix : 0, py ? (iy == 0 ? 0 : 2) : 1, px ? (ix == 0 ? 0 : 2) : 1});
  return taps;
}

struct ConvSpec {
  std::string name;
  Kind kind;
  int ksize;             // 3, 1, or 2 (= ConvTranspose phase set)
  const float* in0;      // source 0
  int cs0, cin0, cin0_pad, H0, W0;
  const float* in1 = nullptr;  // optional second K source (1x1)
  int cs1 = 0, cin1 = 0, cin1_pad = 0, s1 = 1, H1 = 0, W1 = 0;
  const float* res = nullptr;
  int csr = 0;
  float* out;
  int cso, cout, nstore, Ho, Wo;
  int relu;
  bool desc_branch;
};

// conv2_mfma_kernel (round 5) takes a launch with one K source whose workgroups store all of their N channels as float4s
static bool conv_is_lean(const fpc_ctx* c, const Op& op) {
  const KindInfo& k = g_kinds[op.kind];
  const ConvArgs& a = op.args;
  return c->opt.conv_lean && lean_kind(op.kind) && a.nchunk1 == 0 && a.nstore == op.grid_y * (k.WN * k.NB * 32) && a.cso % 4 == 0 &&
         (!a.res || a.csr % 4 == 0);
}

static void add_conv(fpc_ctx* c, const ConvSpec& s, size_t* blob_off) {
  const KindInfo& k = g_kinds[s.kind];
  Op op;
  op.type = OP_CONV;
  op.name = s.name;
  op.kind = s.kind;
  op.descriptor_branch = s.desc_branch;
  ConvArgs& a = op.args;
  const int N = k.WN * k.NB * 32;
  const int nbt = (s.cout + N - 1) / N * (N / 32);
  op.grid_y = nbt * 32 / N;
  a.in0 = s.in0; a.cs0 = s.cs0; a.nchunk0 = s.cin0_pad / k.KC; a.H = s.H0; a.W = s.W0;
  a.in1 = s.in1; a.cs1 = s.cs1; a.nchunk1 = s.in1 ? s.cin1_pad / k.KC : 0; a.s1 = s.s1; a.H1 = s.H1; a.W1 = s.W1;
  a.pad = s.ksize == 3 ? 1 : 0;
  a.res = s.res; a.csr = s.csr;
  a.out = s.out; a.cso = s.cso; a.nstore = s.nstore; a.relu = s.relu; a.nbt = nbt;
  const int HWp = (k.TW - 1) * k.S + k.EXT, ROW4 = k.KC / 4 + 1;
  fpc_ctx::ConvW cw;
  const int K8 = k.KC / 8;
  if (s.ksize == 2) {  // ConvTranspose2d(k3, s2, p1, op1): 4 output-parity phases over the INPUT grid
    op.grid_z = 4;
    a.Ho = s.H0;
    a.Wo = s.W0;
    a.OH = s.Ho;
    a.OW = s.Wo;
    a.oys = a.oxs = 2;
    double macs = 0;
    for (int ph = 0; ph < 4; ++ph) {
      ConvSub& sp = a.sub[ph];
      sp.oy0 = ph >> 1;
      sp.ox0 = ph & 1;
      sp.ntaps = 0;
      for (const ConvTTap& t : convt_phase_taps(ph)) sp.tapoff4[sp.ntaps++] = (t.dy * HWp + t.dx) * ROW4;
      reserve(blob_off, cw.w[ph], conv_floats((size_t)a.nchunk0 * sp.ntaps * K8, nbt));
      macs += (double)sp.ntaps;
    }
    op.flops_per_frame = 2.0 * macs * s.H0 * s.W0 * s.cin0 * s.cout;
    op.mfma_flops_per_frame = 2.0 * macs * ((s.H0 + k.TH - 1) / k.TH) * ((s.W0 + k.TW - 1) / k.TW) * (k.WM * k.MB * 32.0) * (a.nchunk0 * k.KC) * (nbt * 32.0);
  } else {
    a.Ho = a.OH = s.Ho;
    a.Wo = a.OW = s.Wo;
    a.oys = a.oxs = 1;
    ConvSub& sp = a.sub[0];
    sp.oy0 = sp.ox0 = 0;
    sp.ntaps = s.ksize * s.ksize;
    for (int ky = 0; ky < s.ksize; ++ky)
      for (int kx = 0; kx < s.ksize; ++kx) sp.tapoff4[ky * s.ksize + kx] = (ky * HWp + kx) * ROW4;
    reserve(blob_off, cw.w[0], conv_floats((size_t)(a.nchunk0 * sp.ntaps + a.nchunk1) * K8, nbt));
    op.flops_per_frame = 2.0 * s.Ho * s.Wo * s.cout * ((double)s.cin0 * sp.ntaps + s.cin1);
    op.mfma_flops_per_frame = 2.0 * ((s.Ho + k.TH - 1) / k.TH) * ((s.Wo + k.TW - 1) / k.TW) * (k.WM * k.MB * 32.0) * (nbt * 32.0) *
                              ((double)a.nchunk0 * k.KC * sp.ntaps + (double)a.nchunk1 * k.KC);
  }
  reserve(blob_off, cw.b, bias_floats(nbt));
  // conv2_mfma_kernel: one K source, every workgroup stores all of its N channels as float4s
  op.lean = conv_is_lean(c, op);
  a.tiles_x = (a.Wo + k.TW - 1) / k.TW;
  a.tiles_y = (a.Ho + k.TH - 1) / k.TH;
  op.bytes_per_frame = 4.0 * ((double)s.cin0 * s.H0 * s.W0 + (s.in1 ? (double)s.cin1 * s.H1 * s.W1 : 0.0) +
                              (s.res ? (double)s.cout * s.Ho * s.Wo : 0.0) + (double)s.cout * s.Ho * s.Wo);
  push_op(c, op, cw);
}

struct BlockSpec {
  std::string prefix;
  BKind kind;
  const float* x;
  int csx, cin, cin_pad, H, W;
  float* out;
  int cso, cout, cout_pad;
  bool proj, desc_branch;
};

// A fused block on instance `kind`: the instance's halo taps, its tiles over the output, the MFMA work they issue
static void tile_block(Op& o, BKind kind) {
  const BKindInfo& k = g_bkinds[kind];
  o.bkind = kind;
  BlockArgs& a = o.bargs;
  const int HWp = (k.TW - 1) * k.S + 3, ROW4 = k.KC / 4 + 1;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) a.tapoff4[ky * 3 + kx] = (ky * HWp + kx) * ROW4;
  a.tiles_x = (a.Wo + k.TW - 1) / k.TW;
  a.tiles_y = (a.Ho + k.TH - 1) / k.TH;
  o.mfma_flops_per_frame = 2.0 * a.tiles_x * a.tiles_y * (k.WM * k.MB * 32.0) * (k.WN * k.NB * 32.0) *
                           ((double)a.nchunk * k.KC * 9 + (a.k8_h + a.k8_x) * 8.0);
}

static void add_block(fpc_ctx* c, const BlockSpec& s, size_t* blob_off) {
  const BKindInfo& k = g_bkinds[s.kind];
  Op op = weight_op(OP_BLOCK, s.prefix + (s.proj ? " [conv1+bn1+relu+conv2+bn2+proj+relu]" : " [conv1+bn1+relu+conv2+bn2+identity+relu]"),
                    s.prefix, s.cin, s.cout, s.desc_branch);
  BlockArgs& a = op.bargs;
  const int nbt = k.WN * k.NB, K8 = k.KC / 8;
  a.x = s.x;
  a.csx = s.csx;
  a.x_bytes = x_bytes(c, s.H, s.W, s.csx, 4);
  a.nchunk = s.cin_pad / k.KC;
  a.H = s.H;
  a.W = s.W;
  a.k8_h = k.CMIDP / 8;
  a.k8_x = s.proj ? s.cin_pad / 8 : 0;   // the kernel walks the projection eight K steps at a time
  if (a.k8_x % 8) { fprintf(stderr, "fpc: fused block %s: projection over %d channels is not a multiple of 64\n", s.prefix.c_str(), s.cin_pad); abort(); }
  a.out = s.out;
  a.cso = s.cso;
  a.Ho = s.H / k.S;
  a.Wo = s.W / k.S;
  a.nstore = s.cout_pad;
  tile_block(op, s.kind);
  fpc_ctx::ConvW cw;
  reserve(blob_off, cw.w[0], conv_floats((size_t)a.nchunk * 9 * K8, nbt));
  reserve(blob_off, cw.b, bias_floats(nbt));
  reserve(blob_off, cw.w[1], conv_floats(a.k8_h + a.k8_x, nbt));
  reserve(blob_off, cw.b2, bias_floats(nbt));
  op.flops_per_frame = 2.0 * a.Ho * a.Wo * s.cout * ((double)s.cin * 9 + s.cout + (s.proj ? s.cin : 0));
  op.bytes_per_frame = 4.0 * ((double)s.cin * s.H * s.W + (double)s.cout * a.Ho * a.Wo);
  push_op(c, op, cw);
}

// The op just added moves to a finer tile (an instance that consumes the same fragments: same KC and channel blocking).
// Half-size tiles double the workgroups of the stride-2 blocks, the transposed convolution and layer_in.1's 1x1: the
// latency of a single frame's layer is one tile's time (20 - 40 tiles per frame on 256 CUs), and a 32-frame batch runs
// 3 - 10 % faster on them too (shorter tail, more workgroups per CU in flight) -- measured, so they serve every call.
// FPC_PLAN_NO_LATENCY_TILES keeps round 1's tiles.
static void retile_block(fpc_ctx* c, BKind small) {
  const BKindInfo &k0 = g_bkinds[c->ops.back().bkind], &k = g_bkinds[small];
  if (k.KC != k0.KC || k.WN * k.NB != k0.WN * k0.NB || k.S != k0.S || k.CMIDP != k0.CMIDP) { c->plan_error = true; return; }
  tile_block(c->ops.back(), small);
}
static void retile_last(fpc_ctx* c, BKind small) {
  if (!c->opt.latency_tiles || c->ops.empty() || c->ops.back().type != OP_BLOCK) return;
  retile_block(c, small);
}
// MFMA rows a fused block issues per frame on instance `k`: its tiles x the M of a tile (padding included)
static long block_rows(BKind k, int Ho, int Wo) {
  const BKindInfo& b = g_bkinds[k];
  return (long)((Ho + b.TH - 1) / b.TH) * ((Wo + b.TW - 1) / b.TW) * (b.WM * b.MB * 32);
}
// Round 6: the op just added moves to `fit` (same fragments, as above) where that instance issues FEWER rows on the matrix
// cores -- layer2.0's 60 x 80 output is 75 tiles of 4 x 16 = 64 full rows instead of 80 tiles of 3 x 20 = 60 rows in M = 64.
// A tie keeps the instance it has.  plan_hash keeps mixing the instance it had: the blob is the same.
// FPC_PLAN_TILES_ROUND5 keeps round 5's tiles.
static void retile_rows(fpc_ctx* c, BKind fit) {
  if (!c->opt.tiles_round6 || c->ops.empty() || c->ops.back().type != OP_BLOCK) return;
  Op& o = c->ops.back();
  if (block_rows(fit, o.bargs.Ho, o.bargs.Wo) >= block_rows(o.bkind, o.bargs.Ho, o.bargs.Wo)) return;
  const BKind had = o.bkind;
  retile_block(c, fit);
  if (!c->plan_error) c->ops.back().hash_bkind = had;
}

static void retile_last(fpc_ctx* c, Kind small) {
  if (!c->opt.latency_tiles || c->ops.empty() || c->ops.back().type != OP_CONV) return;
  const KindInfo &k0 = g_kinds[c->ops.back().kind], &k = g_kinds[small];
  if (k.KC != k0.KC || k.WN * k.NB != k0.WN * k0.NB || k.S != k0.S || k.EXT != k0.EXT) { c->plan_error = true; return; }
  Op& o = c->ops.back();
  o.kind = small;
  ConvArgs& a = o.args;
  const int HWp = (k.TW - 1) * k.S + k.EXT, HWp0 = (k0.TW - 1) * k0.S + k0.EXT, ROW4 = k.KC / 4 + 1;
  for (int z = 0; z < o.grid_z; ++z)
    for (int t = 0; t < a.sub[z].ntaps; ++t) {   // offsets were (dy * HWp0 + dx) * ROW4 with dx < EXT <= HWp0
      const int lin = a.sub[z].tapoff4[t] / ROW4, dy = lin / HWp0, dx = lin - dy * HWp0;
      a.sub[z].tapoff4[t] = (dy * HWp + dx) * ROW4;
    }
  a.tiles_x = (a.Wo + k.TW - 1) / k.TW;
  a.tiles_y = (a.Ho + k.TH - 1) / k.TH;
  o.lean = conv_is_lean(c, o);
}

// A generation-2 128-channel Winograd op (all of its parts, where it is a conv-only launch of several) on the 4 x 16
// latency tile, WK_W16_C128H -- the same fragments: the copy shares the op's regions
static Op half_tile_copy(const Op& op) {
  const WKindInfo& kh = g_wkinds[WK_W16_C128H];
  Op oh = op;
  WBlockArgs& a = oh.wargs;
  oh.wkind = WK_W16_C128H;
  a.tiles_y = (a.H + kh.TH - 1) / kh.TH;
  oh.mfma_flops_per_frame = op.grid_y * wkind_mfma_flops(kh, a.tiles_x * a.tiles_y, a.nchunk, a.k8_h + a.k8_x);
  return oh;
}

// What the fused and the conv-only Winograd ops share: the tensors, the map, instance `k`'s tiles over it
static void fill_wargs(WBlockArgs& a, const WKindInfo& k, const float* x, int csx, int H, int W, float* out, int cso) {
  a.x = x; a.csx = csx;
  a.H = H; a.W = W;
  a.out = out; a.cso = cso;
  a.tiles_x = (W + k.TW - 1) / k.TW;
  a.tiles_y = (H + k.TH - 1) / k.TH;
}

static void add_wblock(fpc_ctx* c, const BlockSpec& s, WKind wk, size_t* blob_off, bool small_only = false) {
  const WKindInfo& k = g_wkinds[wk];
  Op op = weight_op(OP_WBLOCK, s.prefix + (s.proj ? " [winograd conv1+bn1+relu+conv2+bn2+proj+relu]" : " [winograd conv1+bn1+relu+conv2+bn2+identity+relu]"),
                    s.prefix, s.cin, s.cout, s.desc_branch);
  op.wkind = wk;
  WBlockArgs& a = op.wargs;
  fill_wargs(a, k, s.x, s.csx, s.H, s.W, s.out, s.cso);
  a.nchunk = s.cin_pad / k.KC;
  a.dust = nullptr;
  a.dust_in = 0;
  if (k.dust) {
    // the detector's 65 channels: 64 on the MFMAs (this instance's 4 channel groups), channel 64 beside them (W36Dust).
    // Input: 64 k channels through the chunk loop (+ a projection over them), or 65 = 4 chunks + input channel 64
    // (detector.layer.1, identity shortcut).
    if (s.cout != 65 || !(s.cin == 65 ? !s.proj : (s.cin == s.cin_pad && s.cin_pad % 64 == 0 && s.cin_pad <= 256))) { c->plan_error = true; return; }
    a.dust_in = s.cin == 65;
    a.nchunk = a.dust_in ? 4 : s.cin_pad / 16;
  } else if (s.cin_pad % k.KC) { c->plan_error = true; return; }
  a.k8_h = k.CMID / 8;
  a.k8_x = s.proj ? s.cin_pad / 8 : 0;   // the kernel walks the projection four K steps at a time
  if (a.k8_x % 4) { fprintf(stderr, "fpc: winograd block %s: projection over %d channels is not a multiple of 32\n", s.prefix.c_str(), s.cin_pad); abort(); }
  // generations 2, 3 take an even number of chunks of 16, four at least (wblock16_mfma.h, wblock36_mfma.h)
  if (k.gen >= 2 && (a.nchunk < 4 || (a.nchunk & 1))) { c->plan_error = true; return; }
  fpc_ctx::ConvW cw;
  reserve(blob_off, cw.w[0], w1_floats(k, a.nchunk));
  reserve(blob_off, cw.b, bias_floats(k.NBT));
  reserve(blob_off, cw.w[1], w2_floats(k, a.k8_h + a.k8_x));
  reserve(blob_off, cw.b2, bias_floats(k.NBT));
  if (k.dust) reserve(blob_off, cw.w[2], (size_t)W36Dust::floats(a.nchunk));
  op.flops_per_frame = 2.0 * s.H * s.W * s.cout * ((double)s.cin * 9 + s.cout + (s.proj ? s.cin : 0));
  // 16 (36) GEMMs over the tile's Winograd tiles instead of 9 taps over its pixels; then the 1x1 on its pixels
  op.mfma_flops_per_frame = wkind_mfma_flops(k, a.tiles_x * a.tiles_y, a.nchunk, a.k8_h + a.k8_x);
  if (k.dust && a.dust_in) op.mfma_flops_per_frame += 2.0 * a.tiles_x * a.tiles_y * 64.0 * 36 * 16 * 4;   // input channel 64: one K = 4 MFMA per position
  op.bytes_per_frame = 4.0 * ((double)s.cin * s.H * s.W + (double)s.cout * s.H * s.W);
  // What calls of a few frames run instead.  With fragments of its own (`own`, added by the call below with small_only):
  // - the detector's generation-3 instances keep the round-1 instance, as the 64- / 128-channel layers keep generation 2;
  // - generation 3's tile is 256 pixels: a frame has 20 of them at 60 x 80, and the latency of a single frame's layer is
  //   one tile's time.  Calls of a few frames keep generation 2 (16 positions instead of 36), on its 4 x 16 latency
  //   tiles where that instance exists.
  // On the same fragments (`half`): generation 2's 128-channel layer on 4 x 16 tiles -- under small_only the caller's
  // large-call op exists already, and only that instance is added.
  WKind own = WK_COUNT;
  if (c->opt.latency_tiles && k.dust) own = s.cin == 65 ? WK_W816_K24_C72 : WK_W816_K32_C72;
  else if (c->opt.latency_tiles && k.gen == 3) own = s.cout == 64 ? WK_W16_C64 : WK_W16_C128;
  const bool half = wk == WK_W16_C128 && (small_only || c->opt.latency_tiles);
  op.when = small_only ? 1 : (half || own != WK_COUNT) ? 2 : 0;
  if (!(small_only && half)) push_op(c, op, cw);
  if (half) {
    push_op(c, half_tile_copy(op), cw);
    c->ops.back().when = 1;
  }
  if (own != WK_COUNT) add_wblock(c, s, own, blob_off, true);
}

// A 3x3 stride-1 convolution + (folded BN | bias) + ReLU on the Winograd kernel in conv-only form.  Output channels
// n0 .. n0 + CMID - 1 of the layer (a 256-wide layer takes two launches).  `bn`: weights are `prefix`.conv1.weight +
// `prefix`.bn1.* (a ResNetBlock's first half); otherwise `prefix`.weight + `prefix`.bias (the C++ network).
static void add_wconv(fpc_ctx* c, const std::string& prefix, bool bn, WKind wk, const float* x, int csx, int cin, int H,
                      int W, float* out, int cso, int cout, int n0, bool desc_branch, size_t* blob_off) {
  const WKindInfo& k = g_wkinds[wk];
  Op op = weight_op(OP_WBLOCK, prefix + (bn ? ".conv1+bn1+relu [winograd" : " [winograd conv+bias+relu") +
                    (cout > k.CMID ? ", channels " + std::to_string(n0) + ".." + std::to_string(n0 + k.CMID - 1) : std::string()) + "]",
                    prefix, cin, cout, desc_branch);
  op.wkind = wk;
  if (wk == WK_W36PC_C64_8x2) op.hash_wkind = w36_kind(64, H, W, true);   // the same fragments: plan_hash as FPC_PLAN_TILES_ROUND5's
  op.wconv = true;
  op.plain_conv = !bn;
  op.n0 = n0;
  WBlockArgs& a = op.wargs;
  fill_wargs(a, k, x, csx, H, W, out + n0, cso);
  a.nchunk = cin / k.KC;
  a.k8_h = a.k8_x = 0;
  a.conv_only = 1;
  if (k.gen >= 2 && (a.nchunk < 4 || (a.nchunk & 1))) { c->plan_error = true; return; }
  fpc_ctx::ConvW cw;
  reserve(blob_off, cw.w[0], w1_floats(k, a.nchunk));
  reserve(blob_off, cw.b, bias_floats(k.NBT));
  op.flops_per_frame = 2.0 * H * W * (double)k.CMID * cin * 9;
  op.mfma_flops_per_frame = wkind_mfma_flops(k, a.tiles_x * a.tiles_y, a.nchunk, 0);
  op.bytes_per_frame = 4.0 * ((double)cin * H * W + (double)std::min(k.CMID, cout - n0) * H * W);
  const int part = n0 / k.CMID;
  if (k.gen >= 2 && part > 0 && n0 % k.CMID == 0 && cout % k.CMID == 0 && (int)c->ops.size() >= part) {
    // part 1 .. G - 1 of a layer wider than the instance (256 channels as 2 x 128 or 4 x 64): ONE launch computes all
    // parts (gridDim.y = G; the kernel finds part y's fragments and bias y * ysplit_floats behind part 0's and its
    // outputs y * CMID channels behind `out`); this op only carries the part's checkpoint -> fragment packing
    Op& first = c->ops[c->ops.size() - part];
    fpc_ctx::ConvW& cf = c->convw[c->convw.size() - part];
    if (first.wconv && first.prefix == prefix && first.n0 == 0 && first.wkind == wk && first.grid_y == part) {
      const int ys = (int)((cw.w[0].off - cf.w[0].off) / part);
      if (part == 1) first.wargs.ysplit_floats = ys;
      else if (first.wargs.ysplit_floats != ys) { c->plan_error = true; return; }
      first.grid_y = part + 1;
      first.flops_per_frame += op.flops_per_frame;
      first.mfma_flops_per_frame += op.mfma_flops_per_frame;
      first.bytes_per_frame = 4.0 * ((double)cin * H * W + (double)std::min(cout, (part + 1) * k.CMID) * H * W);
      const std::string parts = std::to_string(part + 1) + " parts of " + std::to_string(k.CMID) + " channels";
      first.name = prefix + (bn ? ".conv1+bn1+relu [winograd, " : " [winograd conv+bias+relu, ") + parts + "]";
      op.shadow = true;
    }
  }
  push_op(c, op, cw);
}

// ---- the Python network, layer by layer -------------------------------------------------------
// One row per ResNetBlock, and one for the up-sample: what the layer IS -- its checkpoint prefix, its tensors and their
// channel strides, its real and padded channel counts, its input map and stride -- whatever runs it.  python_layers()
// fills the rows from the context; which kernel instance runs a row is chosen per arithmetic by build_f32_ops,
// build_bf16_ops and build_x3_ops, and by nothing else.
enum LayerId { L_ENC10, L_ENC11, L_ENC20, L_ENC21, L_DET0, L_DET1, L_IN0, L_IN1, L_UP, L_OUT0, L_OUT1, L_COUNT };
struct Layer {
  const char* prefix;
  float* x;              // input [.., csx]: cin channels, padded to cinp, on an H x W map (bf16 elements in FPC_BF16 mode,
  int csx, cin, cinp;    // as every tensor here -- the strides count elements)
  int H, W, stride;
  float* h;              // conv1's output [.., csh], where the block runs as two launches (the fp32 plan)
  int csh;
  float* y;              // output [.., csy]: cout channels, padded to coutp
  int csy, cout, coutp;
  bool proj, desc;       // projection shortcut; descriptor branch (absent without descriptors)
};

static void python_layers(fpc_ctx* c, Layer* net) {
  const int H4 = c->H / 4, W4 = c->W / 4, Hc = c->H / 8, Wc = c->W / 8, H16 = c->H / 16, W16 = c->W / 16;
  // encoder output lives in channels 128..255 of `cat`; the detector's 65 channels are padded to the logits' stride
  float* feat = c->bf16 ? reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(c->cat) + 128) : c->cat + 128;
  const int dc = c->lgcs;
  net[L_ENC10] = {"encoder.layer1.0", c->x0, 64, 64, 64, H4, W4, 1, c->h4, 64, c->x1, 64, 64, 64, true, false};
  net[L_ENC11] = {"encoder.layer1.1", c->x1, 64, 64, 64, H4, W4, 1, c->h4, 64, c->x2, 64, 64, 64, false, false};
  net[L_ENC20] = {"encoder.layer2.0", c->x2, 64, 64, 64, H4, W4, 2, c->h8, 128, c->x3, 128, 128, 128, true, false};
  net[L_ENC21] = {"encoder.layer2.1", c->x3, 128, 128, 128, Hc, Wc, 1, c->h8, 128, feat, 256, 128, 128, false, false};
  net[L_DET0] = {"detector.layer.0", feat, 256, 128, 128, Hc, Wc, 1, c->dh, 72, c->d0, dc, 65, dc, true, false};
  net[L_DET1] = {"detector.layer.1", c->d0, dc, 65, dc, Hc, Wc, 1, c->dh, 72, c->lg, dc, 65, dc, false, false};
  net[L_IN0] = {"descriptor.layer_in.0", feat, 256, 128, 128, Hc, Wc, 2, c->h16, 256, c->y16a, 256, 256, 256, true, true};
  net[L_IN1] = {"descriptor.layer_in.1", c->y16a, 256, 256, 256, H16, W16, 1, c->h16, 256, c->y16b, 256, 256, 256, false, true};
  // ConvTranspose2d(k3, s2, p1, op1) + bn + relu: the H16 x W16 map doubles into channels 0..127 of `cat`
  net[L_UP] = {"descriptor.up_sample", c->y16b, 256, 256, 256, H16, W16, 1, nullptr, 0, c->cat, 256, 128, 128, false, true};
  net[L_OUT0] = {"descriptor.layer_out.0", c->cat, 256, 256, 256, Hc, Wc, 1, c->lo_h, 128, c->lo0, 128, 128, 128, true, true};
  net[L_OUT1] = {"descriptor.layer_out.1", c->lo0, 128, 128, 128, Hc, Wc, 1, c->lo_h, 128, c->desc_map, 128, 128, 128, false, true};
}
static int layer_count(const fpc_ctx* c) { return c->cfg.descriptor_enabled ? (int)L_COUNT : (int)L_IN0; }

static BlockSpec block_spec(const Layer& L, BKind kind) {
  return {L.prefix, kind, L.x, L.csx, L.cin, L.cinp, L.H, L.W, L.y, L.csy, L.cout, L.coutp, L.proj, L.desc};
}
// One OP_CONV of `L`: `cin` channels (padded to `cinp`) of `in` on an H x W map -> L's output channels in `out`
static ConvSpec conv_spec(const Layer& L, const char* role, Kind kind, int ksize, const float* in, int cs,
                          int cin, int cinp, int H, int W, float* out, int cso, int Ho, int Wo, int relu) {
  ConvSpec s{};
  s.name = std::string(L.prefix) + role;
  s.kind = kind; s.ksize = ksize;
  s.in0 = in; s.cs0 = cs; s.cin0 = cin; s.cin0_pad = cinp; s.H0 = H; s.W0 = W;
  s.out = out; s.cso = cso; s.cout = L.cout; s.nstore = L.coutp; s.Ho = Ho; s.Wo = Wo; s.relu = relu;
  s.desc_branch = L.desc;
  return s;
}
// a block's first half, conv1 + bn1 + relu: x -> h
static ConvSpec conv1_spec(const Layer& L, Kind kind) {
  return conv_spec(L, ".conv1+bn1+relu", kind, 3, L.x, L.csx, L.cin, L.cinp, L.H, L.W, L.h, L.csh, L.H / L.stride, L.W / L.stride, 1);
}
// ... its second half, conv2 + bn2 + shortcut + relu: h -> y, the projection over x as a second K source or x as the
// residual -- or `shortcut`, a projection computed apart (laid out as h), as the residual
static ConvSpec conv2_spec(const Layer& L, Kind kind, const float* shortcut = nullptr) {
  const int Ho = L.H / L.stride, Wo = L.W / L.stride;
  ConvSpec t = conv_spec(L, shortcut ? ".conv2+bn2+shortcut+relu" : L.proj ? ".conv2+bn2+proj+relu" : ".conv2+bn2+identity+relu", kind, 1,
                         L.h, L.csh, L.cout, L.coutp, Ho, Wo, L.y, L.csy, Ho, Wo, 1);
  if (shortcut) {
    t.res = shortcut; t.csr = L.csh;
  } else if (L.proj) {
    t.in1 = L.x; t.cs1 = L.csx; t.cin1 = L.cin; t.cin1_pad = L.cinp; t.s1 = L.stride; t.H1 = L.H; t.W1 = L.W;
  } else {
    t.res = L.x; t.csr = L.csx;
  }
  return t;
}
// ... its projection shortcut as a launch of its own: x -> out, laid out as h
static ConvSpec shortcut_spec(const Layer& L, Kind kind, float* out) {
  return conv_spec(L, ".identity_downsample", kind, 1, L.x, L.csx, L.cin, L.cinp, L.H, L.W, out, L.csh, L.H, L.W, 0);
}
// the up-sample (frames are multiples of 16 with descriptors on: the doubled map is the 1/8 map)
static ConvSpec upsample_spec(const Layer& L, Kind kind) {
  return conv_spec(L, "+bn+relu", kind, 2, L.x, L.csx, L.cin, L.cinp, L.H, L.W, L.y, L.csy, 2 * L.H, 2 * L.W, 1);
}

// ---- bf16 plan (block_bf16.h) ---------------------------------------------------------------
struct FBlockSpec {
  std::string prefix;
  FKind kind;
  const void* x;
  int csx, in_f32, cin, cin_pad, H, W;
  void* out;
  int cso, out_f32, cout;
  bool proj, desc_branch;
};
// (FPC_BF16 keeps bf16 tensors but for the logits; the split modes the fp32 plan's buffers, all fp32)
static FBlockSpec fblock_spec(const fpc_ctx* c, const Layer& L, FKind kind) {
  return {L.prefix, kind, L.x, L.csx, c->split, L.cin, L.cinp, L.H, L.W, L.y, L.csy, c->split || L.y == c->lg, L.cout, L.proj, L.desc};
}

static const char* fplanes_tag(const FKindInfo& k) { return k.planes == 3 ? "3xbf16" : k.planes == 2 ? "2xfp16" : "bf16"; }
// split operands: six bf16 (three fp16) MFMAs per product
static double fplanes_mfmas(const FKindInfo& k) { return k.planes == 3 ? 6.0 : k.planes == 2 ? 3.0 : 1.0; }
// halo offset of tap (dy, dx) in 16-byte units
// (halo row pitch: block_bf16_kernel pads it for its bank-conflict-free pixel order, block_bf16.h)
static int ftap_off(const FKindInfo& k, int dy, int dx) {
  const int HWp = k.planes == 1 ? bf_halo_pitch(k.TH, k.TW, k.S, k.EXT) : (k.TW - 1) * k.S + k.EXT, ROW16 = k.KC / 8 + 1;
  return (dy * HWp + dx) * ROW16;
}
// What every OP_BF16 launch's arguments share: the tensors, the K chunks, the Ho x Wo grid instance `k`'s tiles walk and
// where its points land in the output (every `os`-th pixel; a caller with parity phases adds oy0 / ox0)
static void fill_fargs(BlockBfArgs& a, const FKindInfo& k, const void* x, int csx, int in_f32, int cin_pad, int H, int W,
                       void* out, int cso, int out_f32, int Ho, int Wo, int os) {
  a.x = x; a.csx = csx; a.in_f32 = in_f32;
  a.nchunk = cin_pad / k.KC;
  a.H = H; a.W = W;
  a.out = out; a.cso = cso; a.out_f32 = out_f32;
  a.Ho = Ho; a.Wo = Wo; a.OH = os * Ho; a.OW = os * Wo; a.oys = a.oxs = os;
  a.tiles_x = (Wo + k.TW - 1) / k.TW;
  a.tiles_y = (Ho + k.TH - 1) / k.TH;
}
// ... a ksize x ksize window's taps
static void fill_ftaps(BlockBfArgs& a, const FKindInfo& k, int ksize) {
  a.pad = ksize / 2;
  a.ntaps = ksize * ksize;
  for (int ky = 0; ky < ksize; ++ky)
    for (int kx = 0; kx < ksize; ++kx) a.tapoff16[ky * ksize + kx] = ftap_off(k, ky, kx);
}

static void add_fblock(fpc_ctx* c, const FBlockSpec& s, size_t* blob_off) {
  if (s.kind >= FK_COUNT) { c->plan_error = true; return; }
  const FKindInfo& k = g_fkinds[s.kind];
  Op op = weight_op(OP_BF16, s.prefix + " [" + fplanes_tag(k) + (s.proj ? " conv1+bn1+relu+conv2+bn2+proj+relu]" : " conv1+bn1+relu+conv2+bn2+identity+relu]"),
                    s.prefix, s.cin, s.cout, s.desc_branch);
  op.fkind = s.kind;
  BlockBfArgs& a = op.fargs;
  const int nbt = k.WN * k.NB, K16 = k.KC / 16;
  fill_fargs(a, k, s.x, s.csx, s.in_f32, s.cin_pad, s.H, s.W, s.out, s.cso, s.out_f32, s.H / k.S, s.W / k.S, 1);
  a.x_bytes = x_bytes(c, s.H, s.W, s.csx, 2);
  // block_bf16_one_kernel: the single chunk is a compile-time fact of the instance (block_bf16.h)
  if (strstr(k.symbol, "block_bf16_one_kernel") && a.nchunk != 1) { c->plan_error = true; return; }
  if (strstr(k.symbol, "block_bf16_two_kernel") && a.nchunk != 2) { c->plan_error = true; return; }
  fill_ftaps(a, k, 3);
  a.k16_h = k.CMIDP / 16;
  a.k16_x = s.proj ? s.cin_pad / 16 : 0;
  fpc_ctx::ConvW cw;
  // FPC_BF16 (planes == 1): the shortcut's fragments (projection, or the identity as a unit matrix) follow each chunk's
  // conv1 fragments in the w1 stream as a tenth tap (block_bf16.h), and w2 holds conv2 only
  const bool sc_in_w1 = k.planes == 1;
  reserve(blob_off, cw.w[0], conv_bf16_floats((size_t)a.nchunk * (sc_in_w1 ? 10 : 9) * K16, nbt, k.planes));
  reserve(blob_off, cw.b, bias_floats(nbt));
  reserve(blob_off, cw.w[1], conv_bf16_floats(a.k16_h + (sc_in_w1 ? 0 : a.k16_x), nbt, k.planes));
  reserve(blob_off, cw.b2, bias_floats(nbt));
  op.flops_per_frame = 2.0 * a.Ho * a.Wo * s.cout * ((double)s.cin * 9 + s.cout + (s.proj ? s.cin : 0));
  op.mfma_flops_per_frame = fplanes_mfmas(k) * 2.0 * a.tiles_x * a.tiles_y * (k.WM * k.MB * 32.0) * (nbt * 32.0) *
                            ((double)a.nchunk * k.KC * 9 + (a.k16_h + (sc_in_w1 ? s.cin_pad / 16 : a.k16_x)) * 16.0);
  op.bytes_per_frame = (double)s.cin * s.H * s.W * ((s.in_f32 || k.planes > 1) ? 4.0 : 2.0) +
                       (double)s.cout * a.Ho * a.Wo * ((s.out_f32 || k.planes > 1) ? 4.0 : 2.0);
  push_op(c, op, cw);
}

// The up-sample, ConvTranspose2d(k3, s2, p1, op1) + bn + relu, as four output-parity phases: one launch each, or all in one
static void add_fconvT(fpc_ctx* c, FKind kind, const Layer& L, size_t* blob_off) {
  if (kind >= FK_COUNT) { c->plan_error = true; return; }
  const FKindInfo& k = g_fkinds[kind];
  const int nbt = k.WN * k.NB, K16 = k.KC / 16, H = L.H, W = L.W, cin = L.cin, cout = L.cout;
  // round 5: ONE launch (convt_bf16.h) -- a workgroup stages a tile's halo chunk once and issues all nine taps on it, the
  // four parities' accumulators side by side; gridDim.y = the output-channel parts
  const bool fused = strstr(k.symbol, "convt_bf16_kernel") != nullptr;
  if (fused && (cin % k.KC != 0 || cout != k.CMIDP)) { c->plan_error = true; return; }
  for (int ph = fused ? 4 : 0; ph < (fused ? 5 : 4); ++ph) {   // phase 4: all four
    Op op = weight_op(OP_BF16, std::string(L.prefix) + "+bn+relu [" + fplanes_tag(k) + (fused ? ", four parities in one launch]" : " phase " + std::to_string(ph) + "]"),
                      L.prefix, cin, cout, L.desc);
    op.fkind = kind;
    op.phase = ph;
    BlockBfArgs& a = op.fargs;
    fill_fargs(a, k, L.x, L.csx, 0, cin, H, W, L.y, L.csy, 0, H, W, 2);
    a.x_bytes = x_bytes(c, H, W, L.csx, 2);
    a.pad = 0;
    a.conv_only = 1;
    fpc_ctx::ConvW cw;
    if (fused) {
      op.grid_y = k.CMIDP / (k.WN * 32);
      a.ntaps = 9;
      reserve(blob_off, cw.w[0], conv_bf16_floats((size_t)(cin / 16) * 9, k.CMIDP / 32, 1));   // pack_conv_bf16 with KC = 16: [step of 16 channels][tap][32-channel block][lane]
      reserve(blob_off, cw.b, (size_t)k.CMIDP);
      op.flops_per_frame = 2.0 * 9 * H * W * cin * cout;
      op.mfma_flops_per_frame = 2.0 * 9 * a.tiles_x * a.tiles_y * (k.TH * k.TW) * (double)cin * k.CMIDP;
      op.bytes_per_frame = 2.0 * ((double)cin * H * W + 4.0 * cout * H * W);
    } else {
      a.ntaps = 0;
      for (const ConvTTap& t : convt_phase_taps(ph)) a.tapoff16[a.ntaps++] = ftap_off(k, t.dy, t.dx);
      a.oy0 = ph >> 1;
      a.ox0 = ph & 1;
      reserve(blob_off, cw.w[0], conv_bf16_floats((size_t)a.nchunk * a.ntaps * K16, nbt, k.planes));
      reserve(blob_off, cw.b, bias_floats(nbt));
      op.flops_per_frame = 2.0 * a.ntaps * H * W * cin * cout;
      op.mfma_flops_per_frame = fplanes_mfmas(k) * 2.0 * a.ntaps * a.tiles_x * a.tiles_y * (k.WM * k.MB * 32.0) * (a.nchunk * k.KC) * (nbt * 32.0);
      // the four phases read the same input: a quarter of it is attributed to each, plus the phase's quarter of the output
      op.bytes_per_frame = (k.planes > 1 ? 4.0 : 2.0) * ((double)cin * H * W / 4.0 + (double)cout * H * W);
    }
    push_op(c, op, cw);
  }
}

// The rows on the bf16 / split-operand instances `kinds`, one per row
static void add_fnet(fpc_ctx* c, const Layer* net, const FKind* kinds, size_t* bo) {
  for (int l = 0; l < layer_count(c); ++l) {
    if (l == L_UP) add_fconvT(c, kinds[l], net[l], bo);
    else add_fblock(c, fblock_spec(c, net[l], kinds[l]), bo);
    if (l != L_DET1) continue;
    if (c->bf16) c->ops.back().fused_softmax_capable = c->opt.fuse_softmax;
    push_op(c, OP_SOFTMAX, "exp-softmax+depth_to_space+threshold");
  }
}

static void build_bf16_ops(fpc_ctx* c, const Layer* net, size_t* bo) {
  FKind kinds[L_COUNT];
  // (layer1 measured the same 0.53 ms per 64 HD frames on 8 x 16 tiles of 2 x 2 waves x (2 x 1) blocks, 16 x 16 tiles of
  // 4 x 1 waves x (2 x 2) and 8 x 16 tiles of 2 x 1 waves x (2 x 2): not a matter of the blocking;
  // single-wave workgroups (4 x 16 tiles, 1 x 1 waves x (2 x 2) blocks: no barrier waits at all) measured 0.55 ms: not
  // the barriers either.  What these kernels run into is operand delivery: at full MFMA rate a CU's four SIMDs would
  // pull 64 B/clk of weight fragments from L2 and 64 B/clk of pixels from LDS for a 2 x 2 register blocking.)
  kinds[L_ENC10] = kinds[L_ENC11] = FK_F816_s1_K64_C64;
  kinds[L_ENC20] = FK_F620_s2_K64_C128;
  kinds[L_ENC21] = FK_F816_s1_K128_C128;
  // detector.layer.0 on the 2 x 2 blocking of the 128-wide layers (N = 128 for 65 channels: a quarter of the MFMAs on
  // zeros, but four MFMAs per four operand fetches instead of three per four: 0.47 -> 0.40 ms per 64 HD frames);
  // layer.1 (K = 80) measured the same on both shapes and keeps the narrower one
  kinds[L_DET0] = FK_F816_s1_K128_C80w;
  kinds[L_DET1] = FK_F816_s1_K80_C80;
  kinds[L_IN0] = FK_F320_s2_K128_C256;
  kinds[L_IN1] = FK_F416_s1_K128_C256;
  kinds[L_UP] = c->opt.convt_fused ? FK_F816_ctf_K64_C128 : FK_F816_ct_K64_C128;
  kinds[L_OUT0] = FK_F816_s1_K64_C128;
  // (the descriptor map is bf16 as well -- round 3: descriptor16_kernel<8, true> reads it, fpc_forward / the tap convert it)
  kinds[L_OUT1] = FK_F816_s1_K128_C128;
  add_fnet(c, net, kinds, bo);
}

// the fp16 twin of a bf16x3 instance (rows H* follow rows S* in the same order in FPC_BF16_KINDS)
static FKind split_kind(const fpc_ctx* c, FKind s);

// dtype = FPC_F32_SPLIT: the fp32 plan's buffers (all fp32), every ResNetBlock / ConvTranspose on block_x3_kernel
static void build_x3_ops(fpc_ctx* c, const Layer* net, size_t* bo) {
  FKind kinds[L_COUNT];
  kinds[L_ENC10] = kinds[L_ENC11] = FK_S816_s1_K64_C64;
  kinds[L_ENC20] = FK_S620_s2_K16_C128;
  kinds[L_ENC21] = kinds[L_OUT0] = kinds[L_OUT1] = FK_S620_s1_K64_C128;
  kinds[L_DET0] = FK_S620_s1_K64_C80;
  kinds[L_DET1] = FK_S620_s1_K16_C80;
  kinds[L_IN0] = FK_S320_s2_K16_C256;
  kinds[L_IN1] = FK_S320_s1_K64_C256;
  kinds[L_UP] = FK_S620_ct_K64_C128;
  for (FKind& k : kinds) k = split_kind(c, k);
  add_fnet(c, net, kinds, bo);
}

// ---- the reference's C++ network (superpoint::SPModel, cpp/src/model.cc) -----------------------------
// A plain Conv2d + bias (+ ReLU) on the split-operand kernel (conv_only) -- dtype FPC_F32_SPLIT
static void add_fconv(fpc_ctx* c, FKind kind, const std::string& prefix, const float* x, int csx, int cin, int cin_pad,
                      int H, int W, float* out, int cso, int cout, int ksize, bool relu, bool desc_branch,
                      size_t* blob_off) {
  if (kind >= FK_COUNT) { c->plan_error = true; return; }
  const FKindInfo& k = g_fkinds[kind];
  const int nbt = k.WN * k.NB, K16 = k.KC / 16;
  Op op = weight_op(OP_BF16, prefix + " [" + fplanes_tag(k) + " conv+bias" + (relu ? "+relu]" : "]"), prefix, cin, cout, desc_branch);
  op.fkind = kind;
  op.plain_conv = true;
  op.ksize = ksize;
  BlockBfArgs& a = op.fargs;
  fill_fargs(a, k, x, csx, 1, cin_pad, H, W, out, cso, 1, H, W, 1);
  fill_ftaps(a, k, ksize);
  a.conv_only = 1;
  a.norelu = relu ? 0 : 1;
  fpc_ctx::ConvW cw;
  reserve(blob_off, cw.w[0], conv_bf16_floats((size_t)a.nchunk * a.ntaps * K16, nbt, k.planes));
  reserve(blob_off, cw.b, bias_floats(nbt));
  op.flops_per_frame = 2.0 * a.ntaps * H * W * (double)cin * cout;
  op.mfma_flops_per_frame = fplanes_mfmas(k) * 2.0 * a.ntaps * a.tiles_x * a.tiles_y * (k.WM * k.MB * 32.0) * (a.nchunk * k.KC) * (nbt * 32.0);
  op.bytes_per_frame = 4.0 * ((double)cin * H * W + (double)cout * H * W);
  push_op(c, op, cw);
}

static int build_vgg_plan(fpc_ctx* c) {
  const int H = c->H, W = c->W, B = c->B, Hc = H / 8, Wc = W / 8;
  const size_t npix8 = (size_t)B * Hc * Wc;
  if (!c->split && c->opt.winograd) {
    // Where generation 2 runs the full-resolution 64-channel layers -- this network's widest tensors, 256 bytes per frame
    // pixel -- every frame it is handed must lie in its reach (w16_frames_in_reach).  A plan that runs it in every call
    // (FPC_PLAN_WINOGRAD_GEN2; generation 3 with a frame too large for W36_MARKER) addresses the whole batch from frame 0:
    // refused here, before anything is allocated, where max_batch frames do not fit.  The default plan runs it only in
    // calls of a few frames, from the call's frame 0: a call of more frames than fit takes the batch plan instead.
    const int reach = w16_frames_in_reach(H, W, 64);
    const bool every_call = c->opt.winograd_gen == 2 || (c->opt.winograd_gen == 3 && !w36_fits(B, H, W, 64, 64));
    if (every_call && B > reach) return FPC_E_INVALID;
    if (c->opt.winograd_gen == 3 && c->opt.latency_tiles) c->small_reach = reach;
  }
  Carver cv(c);
  // activations: one buffer per tensor (sub-batches of one call run different layers at the same time)
  const int ah[4] = {H, H / 2, H / 4, Hc}, aw[4] = {W, W / 2, W / 4, Wc}, ac[4] = {64, 64, 128, 128};
  float *act_a[4], *act_b[4], *act_p[3], *det_a, *desc_a;
  for (int i = 0; i < 4; ++i) {
    cv.into(&act_a[i], (size_t)B * ah[i] * aw[i] * ac[i]);
    cv.into(&act_b[i], (size_t)B * ah[i] * aw[i] * ac[i]);
    if (i < 3) cv.into(&act_p[i], (size_t)B * ah[i + 1] * aw[i + 1] * ac[i]);
  }
  cv.into(&det_a, npix8 * 256); cv.into(&desc_a, npix8 * 256);
  cv.into(&c->lg, npix8 * 80); cv.into(&c->desc_map, npix8 * 256); cv.into(&c->desc_in_nhwc, npix8 * 256);
  if (int rc = carve_results(c, cv)) return rc;
  // what fpc_read_activation serves: superpoint::SPModel's modules (cpp/src/model.cc).  "det_b" is the logits; "desc_b" the
  // descriptor map as l2norm256_kernel leaves it (normalised in place)
  static const char* const enc_names[4][3] = {{"conv0_a", "conv0_b", "pool0"}, {"conv1_a", "conv1_b", "pool1"},
                                              {"conv2_a", "conv2_b", "pool2"}, {"conv3_a", "conv3_b", nullptr}};
  c->vtaps.clear();
  for (int i = 0; i < 4; ++i) {
    c->vtaps.push_back({enc_names[i][0], act_a[i], ac[i], ac[i], ah[i], aw[i]});
    c->vtaps.push_back({enc_names[i][1], act_b[i], ac[i], ac[i], ah[i], aw[i]});
    if (i < 3) c->vtaps.push_back({enc_names[i][2], act_p[i], ac[i], ac[i], ah[i + 1], aw[i + 1]});
  }
  c->vtaps.push_back({"det_a", det_a, 256, 256, Hc, Wc});
  c->vtaps.push_back({"det_b", c->lg, c->lgcs, 65, Hc, Wc});
  if (c->cfg.descriptor_enabled) {
    c->vtaps.push_back({"desc_a", desc_a, 256, 256, Hc, Wc});
    c->vtaps.push_back({"desc_b", c->desc_map, 256, 256, Hc, Wc});
  }

  size_t bo = BLOB_HEADER_FLOATS;
  c->ops.clear();
  c->convw.clear();
  auto conv = [&](const std::string& prefix, const float* x, int cin, int Hx, int Wx, float* out, int cso, int cout,
                  int ksize, bool relu, bool desc) {
    if (c->split) {
      FKind fk;
      if (ksize == 3) fk = cout == 64 ? split_kind(c, FK_S816_s1_K64_C64) : cout == 128 ? split_kind(c, FK_S620_s1_K64_C128) : split_kind(c, FK_S320_s1_K64_C256);
      else fk = cout == 65 ? split_kind(c, FK_S620_1x1_K64_C80) : split_kind(c, FK_S320_1x1_K64_C256);
      add_fconv(c, fk, prefix, x, cin, cin, cin, Hx, Wx, out, cso, cout, ksize, relu, desc, &bo);
      return;
    }
    if (ksize == 3 && relu && c->opt.winograd) {  // Winograd F(2x2,3x3), conv-only; 256 outputs = two 128-channel launches
      const WKind wk2 = c->opt.winograd_gen >= 2 ? (cout == 64 ? WK_W16_C64 : WK_W16_C128) : (cout == 64 ? WK_W816_K32_C64 : WK_W816_K32_C128);
      auto add = [&](WKind wk, int when) {
        const size_t i0 = c->ops.size();
        for (int n0 = 0; n0 < cout; n0 += g_wkinds[wk].CMID)
          add_wconv(c, prefix, false, wk, x, cin, cin, Hx, Wx, out, cso, cout, n0, desc, &bo);
        mark_when(c, i0, when);
      };
      if (c->opt.winograd_gen == 3 && w36_fits(c->B, Hx, Wx, cin, cso) && cin % 32 == 0 && cin >= 64) {
        // round 4: F(4x4,3x3) for the C++ network's 3x3 layers too (the conv-only form of wblock36_kernel; 256 outputs in
        // parts), with generation 2 -- fragments of its own -- for calls of a few frames, as the Python network's blocks
        // (priced for a 32-frame call whatever max_batch is: the packed layout must not depend on it -- contexts of
        // different max_batch exchange blobs)
        const int part = w36_conv_part(cout, ((Hx + 15) / 16) * ((Wx + 15) / 16) * 32, 256);
        add(w36_kind(part, Hx, Wx, c->opt.w36_paired), c->opt.latency_tiles ? 2 : 0);
        if (c->opt.latency_tiles) add(wk2, 1);
      } else {
        add(wk2, 0);
      }
      return;
    }
    ConvSpec s{};
    s.name = prefix + (relu ? " [conv+bias+relu]" : " [conv+bias]");
    if (ksize == 3) s.kind = cout == 64 ? K_T816_3x3_K64_N64 : K_T620_3x3_K64_N128;
    else s.kind = cout == 65 ? K_T620_1x1_K64_N96 : K_T620_1x1_K64_N128;
    s.ksize = ksize;
    s.in0 = x; s.cs0 = cin; s.cin0 = cin; s.cin0_pad = cin; s.H0 = Hx; s.W0 = Wx;
    s.out = out; s.cso = cso; s.cout = cout; s.nstore = cout == 65 ? cso : cout; s.Ho = Hx; s.Wo = Wx; s.relu = relu ? 1 : 0;
    s.desc_branch = desc;
    add_conv(c, s, &bo);
    c->ops.back().prefix = prefix;
    c->ops.back().plain_conv = true;
    c->ops.back().ksize = ksize;
    c->ops.back().cin = cin;
    c->ops.back().cout = cout;
  };
  const float* x = nullptr;
  for (int i = 0; i < 4; ++i) {
    const std::string pa = "encoder_conv" + std::to_string(i) + "_a", pb = "encoder_conv" + std::to_string(i) + "_b";
    float* a = act_a[i];
    float* b = act_b[i];
    if (i == 0) {  // Conv2d(1, 64): K = 9, plain FMAs
      Op& op = push_op(c, OP_VCONV0, pa + " [conv+bias+relu, 1 input channel]");
      op.prefix = pa;
      op.pout = a;
      op.pH = H; op.pW = W;
      op.flops_per_frame = 2.0 * H * W * 64 * 9;
      op.bytes_per_frame = 4.0 * ((double)H * W + 64.0 * H * W);
      c->vconv0_off = bo;
      bo += 640;
    } else {
      conv(pa, x, ac[i - 1], ah[i], aw[i], a, ac[i], ac[i], 3, true, false);
    }
    conv(pb, a, ac[i], ah[i], aw[i], b, ac[i], ac[i], 3, true, false);
    if (i < 3) {
      Op& op = push_op(c, OP_POOL2, "max_pool2d(2,2) after " + pb);
      op.pin = b;
      op.pout = act_p[i];
      op.pH = ah[i]; op.pW = aw[i]; op.pC = ac[i];
      op.bytes_per_frame = 4.0 * 1.25 * ac[i] * ah[i] * aw[i];
      x = op.pout;
    } else {
      x = b;
    }
  }
  conv("detector_conv_a", x, 128, Hc, Wc, det_a, 256, 256, 3, true, false);
  conv("detector_conv_b", det_a, 256, Hc, Wc, c->lg, c->lgcs, 65, 1, false, false);
  push_op(c, OP_SOFTMAX, "exp-softmax+depth_to_space+threshold");
  if (c->cfg.descriptor_enabled) {
    conv("descriptor_conv_a", x, 128, Hc, Wc, desc_a, 256, 256, 3, true, true);
    conv("descriptor_conv_b", desc_a, 256, Hc, Wc, c->desc_map, 256, 256, 1, false, true);
    Op& op = push_op(c, OP_L2NORM, "descriptor L2 normalisation over channels");
    op.descriptor_branch = true;
    op.pout = c->desc_map;
    op.bytes_per_frame = 4.0 * 2 * 256.0 * Hc * Wc;
  }
  return finish_plan(c, bo);
}

// Rows H* of FPC_BF16_KINDS must mirror rows S* one for one.  (Round 1, gdb.log: with the two H*_1x1 rows still
// missing, the C++ network's 1x1 layers in FPC_F32_SPLIT_F16 mode indexed past the end of g_fkinds, read TW = KC = 0 and
// build_vgg_plan died with SIGFPE in `(W + TW - 1) / TW`.)
static_assert((int)FK_COUNT - (int)FK_H816_s1_K64_C64 == (int)FK_H816_s1_K64_C64 - (int)FK_S816_s1_K64_C64,
              "every S* (bf16x3) instance needs its H* (fp16x2) twin, in the same order");
static FKind split_kind(const fpc_ctx* c, FKind s) {
  if (!c->split_f16) return s;
  const int h = (int)s + ((int)FK_H816_s1_K64_C64 - (int)FK_S816_s1_K64_C64);
  return h >= (int)FK_H816_s1_K64_C64 && h < (int)FK_COUNT ? (FKind)h : FK_COUNT;
}

// ---- fp32 plan: a row as ONE fused launch (direct or Winograd), or as its conv1 / conv2 launches -------------------
struct F32Kinds {
  Kind k3, k1;   // unfused: conv1 (the up-sample's only launch) and conv2
  BKind bk;      // the fused direct block
};

// The Winograd instance of a fused stride-1 block (WK_COUNT: none, the direct block runs it)
static WKind wblock_kind(const fpc_ctx* c, const Layer& L) {
  if (!c->opt.winograd || L.stride != 1) return WK_COUNT;
  const bool fits = w36_fits(c->B, L.H, L.W, L.csx, L.csy);
  // generation 3's projection pass walks x in 16-channel steps, 4 or 8 per pass (wblock36_mfma.h: gemm_over advances
  // by 4): k8_x = cinp / 8 must be a multiple of 8, i.e. cinp of 64 -- true of every layer of both networks; a
  // layer that is not falls back to generation 2 instead of running extra K steps over stale staging rows
  const int gen = c->opt.winograd_gen == 3 && (!fits || (L.proj && L.cinp % 64 != 0)) ? 2 : c->opt.winograd_gen;
  if (L.cinp % 32 == 0 && L.cout == 64) return gen == 3 ? w36_kind(64, L.H, L.W, c->opt.w36_paired) : gen == 2 ? WK_W16_C64 : WK_W816_K32_C64;
  if (L.cinp % 32 == 0 && L.cout == 128) return gen == 3 ? w36_kind(128, L.H, L.W) : gen == 2 ? WK_W16_C128 : WK_W816_K32_C128;
  if (!c->opt.winograd_det) return WK_COUNT;
  if (L.cout == 65 && c->opt.winograd_det_gen3 && c->opt.winograd_gen == 3 && fits &&
      (L.cin == 65 ? !L.proj : (L.cin == L.cinp && L.cinp % 64 == 0 && L.cinp <= 256)))
    return w36_kind(65, L.H, L.W, c->opt.w36_paired);
  if (L.cinp % 32 == 0 && L.coutp == 72) return WK_W816_K32_C72;
  if (L.cinp == 72 && L.coutp == 72) return WK_W816_K24_C72;
  return WK_COUNT;
}

static void add_f32_block(fpc_ctx* c, const Layer& L, const F32Kinds& k, size_t* bo) {
  if (c->opt.fuse_blocks) {
    const WKind wk = wblock_kind(c, L);
    if (wk != WK_COUNT) add_wblock(c, block_spec(L, k.bk), wk, bo);
    else add_block(c, block_spec(L, k.bk), bo);
    return;
  }
  add_conv(c, conv1_spec(L, k.k3), bo);
  add_conv(c, conv2_spec(L, k.k1), bo);
}

// conv1 of `L` as ONE conv-only Winograd launch on `wk`, in parts of that instance's width: x -> h
static void add_wconv1(fpc_ctx* c, const Layer& L, WKind wk, size_t* bo) {
  for (int n0 = 0; n0 < L.cout; n0 += g_wkinds[wk].CMID)
    add_wconv(c, L.prefix, true, wk, L.x, L.csx, L.cin, L.H, L.W, L.h, L.csh, L.cout, n0, L.desc, bo);
}

// descriptor.layer_in.1 of a fused Winograd plan.  256 channels are too wide for the fused Winograd block (accumulators):
// conv1 as two conv-only Winograd launches of 128 output channels each, then conv2 + identity + ReLU as a 1x1 launch (h
// makes one round trip)
static void add_f32_in1(fpc_ctx* c, const Layer& L, const F32Kinds& k, size_t* bo) {
  // Generation 3: FOUR parts of 64 channels (the NB = 1 instance, gridDim.y = 4).  A 30 x 40 map is 6 tiles per
  // frame: 192 tiles x 2 halves were 384 one-tile workgroups = 1.5 rounds of the 256 CUs at the 128-channel tile's
  // time; 192 x 4 = 768 half-as-long tiles are 3 full rounds (64 workgroups per part walk 3 tiles each).
  const bool g3 = c->opt.winograd_gen == 3 && w36_fits(c->B, L.H, L.W, L.csx, L.csy);
  const WKind wk = g3 ? w36_kind(64, L.H, L.W, c->opt.w36_paired, c->opt.tiles_round6) : c->opt.winograd_gen >= 2 ? WK_W16_C128 : WK_W816_K32_C128;
  const int gen = g_wkinds[wk].gen;
  const ConvSpec t = conv2_spec(L, k.k1);
  const size_t ia = c->ops.size();   // [the launch, its shadows, the 1x1]
  add_wconv1(c, L, wk, bo);
  add_conv(c, t, bo);
  retile_last(c, K_T320_1x1_K64_N128);
  if (c->plan_error) return;
  if (gen == 2 && c->opt.latency_tiles) {
    // calls of a few frames: the same two-half launch on 4 x 16 tiles (24 tiles x 2 halves per frame instead of
    // 12 x 2), then the same 1x1 -- 0.10 ms for one frame against 0.16 ms for the fused direct block on 20 tiles
    c->ops[ia].when = 2;
    c->ops.insert(c->ops.begin() + ia + 1, half_tile_copy(c->ops[ia]));
    c->ops[ia + 1].when = 1;
    c->convw.insert(c->convw.begin() + ia + 1, fpc_ctx::ConvW(c->convw[ia]));
  } else if (gen == 3 && c->opt.latency_tiles) {
    // generation 3's fragments have 36 positions: the small-call variant (generation 2 on 4 x 16 tiles, then the same
    // 1x1) gets fragments of its own
    mark_when(c, ia, 2);
    const size_t ib = c->ops.size();
    add_wconv1(c, L, WK_W16_C128, bo);
    add_conv(c, t, bo);
    retile_last(c, K_T320_1x1_K64_N128);
    if (c->plan_error) return;
    c->ops[ib] = half_tile_copy(c->ops[ib]);
    mark_when(c, ib, 1);
  } else if (c->opt.latency_tiles || c->opt.winograd_gen == 1) {
    mark_when(c, ia, 2);
    // a call of a few frames has 12 tiles per frame here: three dependent launches cost more latency than they save
    // work, so small calls take the fused direct block instead (its weights sit in the blob next to the others)
    add_f32_block(c, L, k, bo);
    c->ops.back().when = 1;
  }
}

static void build_f32_ops(fpc_ctx* c, const Layer* net, size_t* bo) {
  const BKind l1kind = c->opt.layer1_t816 ? BK_B816_s1_K64_C64 : BK_B1616_s1_K32_C64;
  F32Kinds kinds[L_COUNT];
  kinds[L_ENC10] = kinds[L_ENC11] = {K_T816_3x3_K64_N64, K_T816_1x1_K64_N64, l1kind};
  kinds[L_ENC20] = {K_T620_3x3s2_K32_N128, K_T620_1x1_K64_N128, BK_B620_s2_K32_C128};
  kinds[L_ENC21] = kinds[L_OUT0] = kinds[L_OUT1] = {K_T620_3x3_K64_N128, K_T620_1x1_K64_N128, BK_B620_s1_K64_C128};
  kinds[L_DET0] = {K_T620_3x3_K64_N96, K_T620_1x1_K72_N96, BK_B620_s1_K64_C72};
  kinds[L_DET1] = {K_T620_3x3_K72_N96, K_T620_1x1_K72_N96, BK_B620_s1_K72_C72};
  kinds[L_IN0] = {K_T620_3x3s2_K32_N128, K_T620_1x1_K64_N128, BK_B320_s2_K32_C256};
  kinds[L_IN1] = {K_T620_3x3_K64_N128, K_T620_1x1_K64_N128, BK_B320_s1_K64_C256};
  kinds[L_UP] = {K_T620_2x2_K64_N128, K_COUNT, BK_COUNT};
  for (int l = 0; l < layer_count(c); ++l) {
    const Layer& L = net[l];
    const F32Kinds& k = kinds[l];
    if (l == L_UP) {
      add_conv(c, upsample_spec(L, k.k3), bo);
      retile_last(c, K_T320_2x2_K64_N128);
    } else if (l == L_DET0 && !c->opt.fuse_blocks) {
      // detector.layer.0: the projection shortcut has K = 128 while conv2 has K = 72 (65 padded):
      // run the shortcut as its own 1x1 and add it as the residual of conv2
      add_conv(c, conv1_spec(L, k.k3), bo);
      add_conv(c, shortcut_spec(L, K_T620_1x1_K64_N96, c->dproj), bo);
      add_conv(c, conv2_spec(L, k.k1, c->dproj), bo);
    } else if (l == L_IN1 && c->opt.fuse_blocks && c->opt.winograd && c->opt.winograd_in1) {
      add_f32_in1(c, L, k, bo);
    } else {
      add_f32_block(c, L, k, bo);
    }
    if (l == L_ENC20 && c->opt.fuse_blocks) {
      retile_last(c, BK_B320_s2_K32_C128);
      retile_rows(c, BK_B416_s2_K32_C128);
    }
    if (l == L_IN0 && c->opt.fuse_blocks) retile_last(c, BK_B310_s2_K32_C256);
    if (l == L_DET1) push_op(c, OP_SOFTMAX, "exp-softmax+depth_to_space+threshold");
  }
}

static int build_plan(fpc_ctx* c) {
  if (c->vgg) return build_vgg_plan(c);
  const int H = c->H, W = c->W, B = c->B;
  const int H2 = H / 2, W2 = W / 2, H4 = H / 4, W4 = W / 4, Hc = H / 8, Wc = W / 8, H16 = H / 16, W16 = W / 16;
  // ---- carve the slab: this network's activations, then what both networks share
  Carver cv(c);
  const size_t npix4 = (size_t)B * H4 * W4, npix8 = (size_t)B * Hc * Wc, npix16 = (size_t)B * H16 * W16;
  cv.into(&c->stem_out, (size_t)B * H2 * W2 * 64);
  cv.into(&c->x0, npix4 * 64); cv.into(&c->h4, npix4 * 64); cv.into(&c->x1, npix4 * 64); cv.into(&c->x2, npix4 * 64);
  cv.into(&c->h8, npix8 * 128); cv.into(&c->x3, npix8 * 128);
  cv.into(&c->cat, npix8 * 256);
  cv.into(&c->dh, npix8 * 72); cv.into(&c->dproj, npix8 * 72);
  cv.into(&c->d0, npix8 * 80); cv.into(&c->lg, npix8 * 80);
  cv.into(&c->h16, npix16 * 256); cv.into(&c->y16a, npix16 * 256); cv.into(&c->y16b, npix16 * 256);
  cv.into(&c->lo_h, npix8 * 128); cv.into(&c->lo0, npix8 * 128);
  cv.into(&c->desc_map, npix8 * 128); cv.into(&c->desc_in_nhwc, npix8 * 128);
  if (int rc = carve_results(c, cv)) return rc;

  // ---- ops
  size_t bo = BLOB_HEADER_FLOATS;  // blob offset in floats (the tag of the packed format comes first)
  c->ops.clear();
  c->convw.clear();
  {
    Op& op = push_op(c, OP_STEM, "encoder.conv1+bn1+relu");
    op.flops_per_frame = 2.0 * H2 * W2 * 64 * 147;  // of the reference's 3-channel convolution, also for gray frames
    op.mfma_flops_per_frame = 2.0 * ((H2 + 15) / 16) * ((W2 + 15) / 16) * 256.0 * 64 * 152;
    op.bytes_per_frame = 4.0 * (double)c->cin * H * W + (c->bf16 ? 2.0 : 4.0) * 64.0 * H4 * W4;   // frame in, pooled map out
    if (c->split || c->bf16)  // stem_pool_x3_kernel: (rows + 1) / 2 K16 steps of six bf16 MFMAs
      op.mfma_flops_per_frame = (c->bf16 ? 1 : c->split_f16 ? 3 : 6) * 2.0 * ((H2 + 15) / 16) * ((W2 + 15) / 16) * 256.0 * 64 * 16.0 * ((c->cin * 7 + 1) / 2);
    if (c->bf16)              // stem_bf16_kernel: 8 x 7 pooled pixels per tile, 8 blocks of 32 pixels x 64 channels x K16 steps
      op.mfma_flops_per_frame = 2.0 * ((H4 + SB2_PH - 1) / SB2_PH) * ((W4 + SB2_PW - 1) / SB2_PW) * 256.0 * 64 * 16.0 * ((c->cin * 7 + 1) / 2);
    c->stem_w_off = bo;
    // + two zero groups: the fused kernel prefetches ahead; the split-operand stem needs 13 steps x 3 planes
    bo += std::max<size_t>((size_t)(STEM_KG + 2) * 2 * 64 * 4, (size_t)13 * 3 * 2 * 64 * 4);
    c->stem_b_off = bo;
    bo += 64;
    push_op(c, OP_POOL, "encoder.max_pool");
  }
  Layer net[L_COUNT];
  python_layers(c, net);
  if (c->bf16) build_bf16_ops(c, net, &bo);
  else if (c->split) build_x3_ops(c, net, &bo);
  else build_f32_ops(c, net, &bo);
  if (int rc = finish_plan(c, bo)) return rc;
  c->stem.wfrag = reinterpret_cast<const float4*>(c->blob + c->stem_w_off);
  c->stem.bias = c->blob + c->stem_b_off;
  c->stem.out = c->stem_out;
  c->stem.H = H; c->stem.W = W; c->stem.Ho = H2; c->stem.Wo = W2;
  c->stem.tiles_x = (W2 + STEM_T - 1) / STEM_T;
  c->stem.tiles_y = (H2 + STEM_T - 1) / STEM_T;
  // round 5: the fp32 stem + pool on stem_pool2_kernel where the conv map's width is whole tiles (VGA, HD, QVGA).  The fragments carry the bias as a K step in EVERY geometry (pack layout revision 4; stem_pool_kernel and
  // stem_kernel skip that step), so the choice is a launch-time one and blobs stay exchangeable between geometries
  c->opt.stem2 = c->opt.stem_lean && !c->bf16 && !c->split && !c->vgg && (c->opt.fuse_stem_pool || c->cin == 1) && H2 % 2 == 0 && W2 % STEM_T == 0;
  return FPC_OK;
}


// ---- the packed blob's tag ----------------------------------------------------------------
// The first 16 words of the blob describe what packed it, so that a blob that travels (fpc_export_packed ->
// fpc_import_packed, the RCCL broadcast) is never interpreted with another layout: magic, ABI version, dtype, arch,
// a hash of the launch plan (kernel instances and fragment offsets of every layer), the blob size.
static uint64_t plan_hash(const fpc_ctx* c) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xff;
      h *= 1099511628211ull;
    }
  };
  mix(FPC_ABI_VERSION); mix(FPC_PACK_LAYOUT_REVISION); mix((uint64_t)c->cfg.dtype); mix((uint64_t)c->cfg.arch); mix((uint64_t)c->cin);
  mix((uint64_t)(c->cfg.descriptor_enabled != 0)); mix(c->blob_floats); mix(c->stem_w_off); mix(c->stem_b_off);
  mix(c->vconv0_off);
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    mix((uint64_t)op.type); mix((uint64_t)op.kind); mix((uint64_t)(op.hash_bkind >= 0 ? (BKind)op.hash_bkind : op.bkind));
    mix((uint64_t)(op.hash_wkind >= 0 ? (WKind)op.hash_wkind : op.wkind)); mix((uint64_t)op.fkind);
    mix((uint64_t)(op.phase + 1)); mix((uint64_t)op.n0);
    for (char ch : op.prefix) mix((uint64_t)(unsigned char)ch);
    const fpc_ctx::ConvW& cw = c->convw[i];
    for (int z = 0; z < 4; ++z) mix(cw.w[z].off);
    mix(cw.b.off); mix(cw.b2.off);
  }
  return h;
}

static void fill_blob_header(const fpc_ctx* c, uint32_t* h) {
  memset(h, 0, BLOB_HEADER_FLOATS * sizeof(uint32_t));
  const uint64_t ph = plan_hash(c);
  h[0] = BLOB_MAGIC; h[1] = FPC_ABI_VERSION; h[2] = (uint32_t)c->cfg.dtype; h[3] = (uint32_t)c->cfg.arch;
  h[4] = (uint32_t)ph; h[5] = (uint32_t)(ph >> 32);
  h[6] = (uint32_t)c->blob_floats; h[7] = (uint32_t)((uint64_t)c->blob_floats >> 32);
  h[8] = 1;  // holds weights
  h[9] = FPC_PACK_LAYOUT_REVISION;
}

static bool check_blob_header(const fpc_ctx* c, const uint32_t* h, std::string* why) {
  uint32_t want[BLOB_HEADER_FLOATS];
  fill_blob_header(c, want);
  static const char* what[10] = {"magic", "ABI version", "dtype", "arch", "launch plan", "launch plan", "size", "size", "weights-present flag",
                                 "fragment-layout revision"};
  for (int i = 0; i < 10; ++i)
    if (h[i] != want[i]) {
      *why = std::string("packed weights do not match this context: ") + what[i] + " differs (the blob was packed by another "
             "build, dtype, arch or plan, or holds no weights)";
      return false;
    }
  return true;
}

// ---- Winograd-domain filters U = G g G^T (x the folded BN scale), in double ------------------------------------
// F(2x2,3x3): 16 positions (generations 1, 2); F(4x4,3x3) on the points 0, +-1, +-2, inf: 36 positions (generation 3).
// U[(n * ci + cc) * P + i * R + j] for output channels n0 .. n0 + nn - 1 of w1 [co][ci][3][3].
static std::vector<double> winograd_filters(const float* w1, int n0, int nn, int ci, const std::vector<double>& scale, int P) {
  static const double G2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  static const double G4[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                  {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
  const int R = P == 36 ? 6 : 4;
  const double(*G)[3] = P == 36 ? G4 : G2;
  std::vector<double> U((size_t)nn * ci * P);
  for (int n = 0; n < nn; ++n)
    for (int cc = 0; cc < ci; ++cc) {
      const float* g = w1 + ((size_t)(n0 + n) * ci + cc) * 9;
      double t[6][3];
      for (int i = 0; i < R; ++i)
        for (int j = 0; j < 3; ++j) t[i][j] = G[i][0] * g[0 * 3 + j] + G[i][1] * g[1 * 3 + j] + G[i][2] * g[2 * 3 + j];
      for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j)
          U[((size_t)n * ci + cc) * P + i * R + j] = (t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2]) * scale[n0 + n];
    }
  return U;
}

// ---- generation-3 Winograd fragments (wblock36_mfma.h): as generation 2's with 36 positions per chunk --------------
static void pack_w36_winograd(const std::vector<double>& U, int nn, int ci, const WKindInfo& k, int nchunk, float* dst) {
  const size_t gstride = w1_floats(k, nchunk) / k.NCG;
  for (int cg = 0; cg < k.NCG; ++cg)
    for (int ch = 0; ch < nchunk; ++ch)
      for (int xi = 0; xi < 36; ++xi)
        for (int lane = 0; lane < 64; ++lane) {
          const int n = 16 * cg + (lane & 15), kq = lane >> 4;
          float* d4 = dst + cg * gstride + (((size_t)ch * 36 + xi) * 64 + lane) * 4;
          for (int j = 0; j < 4; ++j) {
            const int cc = 16 * ch + 4 * kq + j;
            d4[j] = (n < nn && cc < ci) ? (float)U[((size_t)n * ci + cc) * 36 + xi] : 0.f;
          }
        }
}

// ---- generation-2 Winograd fragments (wblock16_mfma.h) ---------------------------------------------
// U: [nn][ci][16] Winograd-domain filters (scaled); dst: [channel group][chunk of 16][position][lane] float4 with
// lane (n = l & 15, kq = l >> 4) holding { U[16 cg + n][16 chunk + 4 kq + j][pos] }, j = 0..3; WPAD zero steps per group.
static void pack_w16_winograd(const std::vector<double>& U, int nn, int ci, const WKindInfo& k, int nchunk, float* dst) {
  const size_t gstride = w1_floats(k, nchunk) / k.NCG;
  for (int cg = 0; cg < k.NCG; ++cg)
    for (int ch = 0; ch < nchunk; ++ch)
      for (int xi = 0; xi < 16; ++xi)
        for (int lane = 0; lane < 64; ++lane) {
          const int n = 16 * cg + (lane & 15), kq = lane >> 4;
          float* d4 = dst + cg * gstride + (((size_t)ch * 16 + xi) * 64 + lane) * 4;
          for (int j = 0; j < 4; ++j) {
            const int cc = 16 * ch + 4 * kq + j;
            d4[j] = (n < nn && cc < ci) ? (float)U[((size_t)n * ci + cc) * 16 + xi] : 0.f;
          }
        }
}

// 1x1 over [h | x]: sources concatenated along K (each a multiple of 16 channels); dst [channel group][step of 16][lane] float4
static void pack_w16_1x1(const std::vector<PackSource>& srcs, int cout, const WKindInfo& k, float* dst) {
  size_t steps = 0;
  for (auto& s : srcs) steps += (size_t)s.cin_pad / 16;
  const int ncg = k.NCG;
  const size_t gstride = w2_floats(k, (int)(2 * steps)) / ncg;
  size_t step0 = 0;
  for (auto& s : srcs) {
    for (int g = 0; g < s.cin_pad / 16; ++g)
      for (int cg = 0; cg < ncg; ++cg)
        for (int lane = 0; lane < 64; ++lane) {
          const int n = 16 * cg + (lane & 15), kq = lane >> 4;
          float* d4 = dst + cg * gstride + ((step0 + g) * 64 + lane) * 4;
          for (int j = 0; j < 4; ++j) {
            const int cc = 16 * g + 4 * kq + j;
            d4[j] = (n < cout && cc < s.cin) ? (float)(s.w(n, cc, 0) * (*s.scale)[n]) : 0.f;
          }
        }
    step0 += (size_t)s.cin_pad / 16;
  }
}

// ---- checkpoint -> blob -----------------------------------------------------------------
static int pack_all_impl(fpc_ctx* c, const TensorMap& m, std::string* missing, bool& range_bad);
static int pack_all(fpc_ctx* c, const TensorMap& m, std::string* missing) {
  bool range_bad = false;
  const int rc = pack_all_impl(c, m, missing, range_bad);
  if (rc == FPC_OK && range_bad) {
    *missing = "a BatchNorm-folded weight exceeds fp16's range (|w| > 65504): FPC_F32_SPLIT_F16 cannot represent it";
    return FPC_E_RANGE;
  }
  if (rc == FPC_OK) fill_blob_header(c, reinterpret_cast<uint32_t*>(c->host_blob.data()));
  return rc;
}
// What every packer below works with: the context and its host blob, the checkpoint, where the first missing key goes.
struct Packer {
  fpc_ctx* c;
  const TensorMap& m;
  std::string* missing;
  bool& range_bad;
  const float* need(const std::string& k, std::initializer_list<int64_t> shp) const {
    if (!has_shape(m, k, shp)) {
      if (missing->empty()) *missing = k;
      return nullptr;
    }
    return m.at(k).data;
  }
  float* at(size_t off) const { return c->host_blob.data() + off; }
  // Writes into an op's region are refused where they are longer than the region: the plan's size function and the packer
  // disagree, and the floats behind the region are another fragment's.  (Never on a correct plan; a load error, not a
  // corrupted neighbour.)
  int fits(const Op& op, const Region& r, size_t n) const {
    if (n <= r.len) return FPC_OK;
    *missing = "internal: " + op.name + " packs " + std::to_string(n) + " floats into a region of " + std::to_string(r.len);
    return FPC_E_INVALID;
  }
  int put(const Op& op, const std::vector<float>& frag, const Region& r) const {
    if (int rc = fits(op, r, frag.size())) return rc;
    memcpy(at(r.off), frag.data(), frag.size() * sizeof(float));
    return FPC_OK;
  }
  template <typename F>
  int fill(const Op& op, const Region& r, int n, F v) const {   // v(0) .. v(n - 1): a bias vector
    if (int rc = fits(op, r, (size_t)std::max(n, 0))) return rc;
    for (int i = 0; i < n; ++i) at(r.off)[i] = (float)v(i);
    return FPC_OK;
  }
};

// A ResNetBlock's checkpoint entries under `p`: conv1, conv2, the optional projection shortcut, their folded BatchNorms
// and the bias behind conv2 (bn2's, plus the projection's bn's)
struct BlockWeights {
  const float *w1 = nullptr, *w2 = nullptr, *wp = nullptr;
  Fold f1, f2, fp;
  std::vector<double> bias;
};
static bool load_block(const Packer& pk, const std::string& p, int ci, int co, bool proj, BlockWeights* b) {
  b->w1 = pk.need(p + ".conv1.weight", {co, ci, 3, 3});
  b->w2 = pk.need(p + ".conv2.weight", {co, co, 1, 1});
  if (!b->w1 || !b->w2 || !fold_bn(pk.m, p + ".bn1", co, &b->f1, pk.missing) || !fold_bn(pk.m, p + ".bn2", co, &b->f2, pk.missing))
    return false;
  b->bias = b->f2.t;
  if (!proj) return true;
  b->wp = pk.need(p + ".identity_downsample.0.weight", {co, ci, 1, 1});
  if (!b->wp || !fold_bn(pk.m, p + ".identity_downsample.1", co, &b->fp, pk.missing)) return false;
  for (int n = 0; n < co; ++n) b->bias[n] += b->fp.t[n];
  return true;
}
// The K sources of a block's 1x1 stage: conv2 over h (padded to `hpad` channels) and, with `xpad`, the projection over x
static std::vector<PackSource> block_1x1_sources(const BlockWeights& b, int ci, int co, int hpad, int xpad) {
  std::vector<PackSource> srcs;
  srcs.push_back({co, hpad, 1, [&b, co](int n, int c_, int) { return (double)b.w2[(size_t)n * co + c_]; }, &b.f2.s});
  if (b.wp && xpad > 0)
    srcs.push_back({ci, xpad, 1, [&b, ci](int n, int c_, int) { return (double)b.wp[(size_t)n * ci + c_]; }, &b.fp.s});
  return srcs;
}

// Generation-1 Winograd fragments (wblock_mfma.h): U [nn][ci][16] as [chunk][xi][k8][nb][lane] float4
static void pack_w8_winograd(const std::vector<double>& U, int nn, int ci, const WKindInfo& k, int nchunk, float* dst) {
  const int nbt = k.NBT, K8 = k.KC / 8;
  for (int ch = 0; ch < nchunk; ++ch)
    for (int xi = 0; xi < 16; ++xi)
      for (int k8 = 0; k8 < K8; ++k8)
        for (int nb = 0; nb < nbt; ++nb)
          for (int lane = 0; lane < 64; ++lane) {
            const int n = nb * 32 + (lane & 31), half = lane >> 5;
            float* d4 = dst + (((((size_t)ch * 16 + xi) * K8 + k8) * nbt + nb) * 64 + lane) * 4;
            for (int j = 0; j < 4; ++j) {
              const int cc = ch * k.KC + k8 * 8 + 4 * half + j;
              d4[j] = (n < nn && cc < ci) ? (float)U[((size_t)n * ci + cc) * 16 + xi] : 0.f;
            }
          }
}
// Winograd-domain filters U of output channels 0 .. nn - 1 in the layout of the op's generation
static void pack_winograd(const std::vector<double>& U, int nn, int ci, const WKindInfo& k, int nchunk, float* dst) {
  if (k.gen == 3) pack_w36_winograd(U, nn, ci, k, nchunk, dst);
  else if (k.gen == 2) pack_w16_winograd(U, nn, ci, k, nchunk, dst);
  else pack_w8_winograd(U, nn, ci, k, nchunk, dst);
}

// superpoint::SPModel: Conv2d weights + biases, no BatchNorm (cpp/src/model.cc:4-58) -- every layer that is not a
// Winograd launch (those: pack_wblock)
static int pack_vgg_convs(const Packer& pk) {
  fpc_ctx* c = pk.c;
  static const std::vector<double> ones(256, 1.0);
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    if (op.type == OP_VCONV0) {
      const float* w = pk.need(op.prefix + ".weight", {64, 1, 3, 3});
      const float* bv = pk.need(op.prefix + ".bias", {64});
      if (!w || !bv) return FPC_E_MISSING_KEY;
      float* dst = pk.at(c->vconv0_off);
      for (int t = 0; t < 9; ++t)
        for (int n = 0; n < 64; ++n) dst[t * 64 + n] = w[n * 9 + t];
      for (int n = 0; n < 64; ++n) dst[576 + n] = bv[n];
      continue;
    }
    if (!op.plain_conv || op.type == OP_WBLOCK) continue;
    const int ci = op.cin, co = op.cout, kk = op.ksize * op.ksize;
    const float* w = pk.need(op.prefix + ".weight", {co, ci, op.ksize, op.ksize});
    const float* bv = pk.need(op.prefix + ".bias", {co});
    if (!w || !bv) return FPC_E_MISSING_KEY;
    const fpc_ctx::ConvW& cw = c->convw[i];
    PackSource src{ci, ci, kk, [&](int n, int cc, int t) { return (double)w[((size_t)n * ci + cc) * kk + t]; }, &ones};
    if (op.type == OP_BF16) {
      const FKindInfo& k = g_fkinds[op.fkind];
      if (int rc = pk.put(op, pack_conv_bf16({src}, co, k.WN * k.NB, k.KC, k.planes, &pk.range_bad), cw.w[0])) return rc;
    } else {
      if (int rc = pk.put(op, pack_conv({src}, co, op.args.nbt, g_kinds[op.kind].KC), cw.w[0])) return rc;
    }
    if (int rc = pk.fill(op, cw.b, co, [&](int n) { return bv[n]; })) return rc;
  }
  return FPC_OK;
}

static int pack_stem(const Packer& pk) {
  fpc_ctx* c = pk.c;
  const float* w = pk.need("encoder.conv1.weight", {64, 3, 7, 7});
  Fold f;
  if (!w || !fold_bn(pk.m, "encoder.bn1", 64, &f, pk.missing)) return FPC_E_MISSING_KEY;
  float* dst = pk.at(c->stem_w_off);
  const int kreal = c->cin * 49, kg = (kreal + 7) / 8;
  if (c->split || c->bf16) {  // stem_pool_x3_kernel: [step][plane][nb][lane] x 8 bf16; k = (row = 2*step + half, kx = j)
    uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);
    const int rows = c->cin * 7, steps = (rows + 1) / 2;
    for (int st = 0; st < steps; ++st)
      for (int nb = 0; nb < 2; ++nb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int row = 2 * st + (lane >> 5), n = nb * 32 + (lane & 31);
            double v = 0.0;
            if (row < rows && j > 0) {     // j = 0: the zero-weight pad (LDS column 0 is one pixel left of the window)
              const int k = row * 7 + j - 1;  // (c, ky, kx = j - 1) flattened exactly as conv1.weight[n]
              if (c->cin == 3) v = (double)w[n * 147 + k];
              else v = (double)w[n * 147 + k] + (double)w[n * 147 + 49 + k] + (double)w[n * 147 + 98 + k];
            }
            const float wv = (float)(v * f.s[n]);
            if (c->bf16) {
              d16[(((size_t)st * 2 + nb) * 64 + lane) * 8 + j] = host_f2bf(wv);
            } else if (c->split_f16) {
              if (!(std::fabs(wv) <= 65504.f)) pk.range_bad = true;
              uint16_t t2[2];
              host_split2_f16(wv, t2);
              for (int pl = 0; pl < 2; ++pl) d16[((((size_t)st * 2 + pl) * 2 + nb) * 64 + lane) * 8 + j] = t2[pl];
            } else {
              uint16_t t3[3];
              host_split3(wv, t3);
              for (int pl = 0; pl < 3; ++pl) d16[((((size_t)st * 3 + pl) * 2 + nb) * 64 + lane) * 8 + j] = t3[pl];
            }
          }
  } else {
    for (int g = 0; g < kg; ++g)
      for (int nb = 0; nb < 2; ++nb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const StemPair sp = stem_pair2(c->cin, g * 4 + j);      // the kernels' K order (kernels_misc.h), bias step included
            const int k = (lane >> 5) ? sp.wb : sp.wa, n = nb * 32 + (lane & 31);
            if (k == STEM_BIAS_TAP) {   // the folded-BN bias as a K step (stem_pool2_kernel: A operand 1.0; the other stem kernels skip the step)
              dst[(((size_t)g * 2 + nb) * 64 + lane) * 4 + j] = (float)f.t[n];
              continue;
            }
            double v = 0.0;
            if (k >= 0 && k < kreal) {
              if (c->cin == 3) v = (double)w[n * 147 + k];
              else  // gray frame == the same plane in all three channels: sum the three filters
                v = (double)w[n * 147 + k] + (double)w[n * 147 + 49 + k] + (double)w[n * 147 + 98 + k];
            }
            dst[(((size_t)g * 2 + nb) * 64 + lane) * 4 + j] = (float)(v * f.s[n]);
          }
  }
  for (int n = 0; n < 64; ++n) pk.at(c->stem_b_off)[n] = (float)f.t[n];
  return FPC_OK;
}

static int pack_wblock(const Packer& pk, const Op& op, const fpc_ctx::ConvW& cw) {
  const WKindInfo& k = g_wkinds[op.wkind];
  const WBlockArgs& a = op.wargs;
  const std::string& p = op.prefix;
  const int ci = op.cin, co = op.cout, nbt = k.NBT, P = k.gen == 3 ? 36 : 16;
  if (op.wconv) {  // conv-only launch: U = G g G^T of output channels n0 .. n0 + CMID - 1
    const float* w1 = pk.need(p + (op.plain_conv ? ".weight" : ".conv1.weight"), {co, ci, 3, 3});
    Fold f1;
    if (!w1) return FPC_E_MISSING_KEY;
    if (op.plain_conv) {
      const float* bv = pk.need(p + ".bias", {co});
      if (!bv) return FPC_E_MISSING_KEY;
      f1.s.assign(co, 1.0);
      f1.t.assign(bv, bv + co);
    } else if (!fold_bn(pk.m, p + ".bn1", co, &f1, pk.missing)) {
      return FPC_E_MISSING_KEY;
    }
    const int nn = std::min(k.CMID, co - op.n0);
    if (int rc = pk.fits(op, cw.w[0], w1_floats(k, a.nchunk))) return rc;
    pack_winograd(winograd_filters(w1, op.n0, nn, ci, f1.s, P), nn, ci, k, a.nchunk, pk.at(cw.w[0].off));
    return pk.fill(op, cw.b, nn, [&](int n) { return f1.t[op.n0 + n]; });
  }
  BlockWeights b;
  if (!load_block(pk, p, ci, co, a.k8_x > 0, &b)) return FPC_E_MISSING_KEY;
  // U = G (g * s) G^T in double, rounded once
  const std::vector<double> U = winograd_filters(b.w1, 0, co, ci, b.f1.s, P);
  if (int rc = pk.fits(op, cw.w[0], w1_floats(k, a.nchunk))) return rc;
  pack_winograd(U, co, ci, k, a.nchunk, pk.at(cw.w[0].off));
  if (int rc = pk.fill(op, cw.b, std::min(co, nbt * 32), [&](int n) { return b.f1.t[n]; })) return rc;
  const std::vector<PackSource> srcs = block_1x1_sources(b, ci, co, a.k8_h * 8, a.k8_x * 8);
  if (k.gen >= 2) {
    if (int rc = pk.fits(op, cw.w[1], w2_floats(k, a.k8_h + a.k8_x))) return rc;
    pack_w16_1x1(srcs, co, k, pk.at(cw.w[1].off));
  } else if (int rc = pk.put(op, pack_conv(srcs, co, nbt, 8), cw.w[1])) {
    return rc;
  }
  if (int rc = pk.fill(op, cw.b2, std::min(co, nbt * 32), [&](int n) { return b.bias[n]; })) return rc;
  if (k.dust) {   // the 65th channel's weights (W36Dust, wblock36_mfma.h)
    if (int rc = pk.fits(op, cw.w[2], (size_t)W36Dust::floats(a.nchunk))) return rc;
    float* d = pk.at(cw.w[2].off);
    for (int n = 0; n < 64; ++n) d[W36Dust::W2ROW + n] = (float)((double)b.w2[(size_t)n * co + 64] * b.f2.s[n]);
    for (int kk = 0; kk < 65; ++kk) d[W36Dust::W2COL + kk] = (float)((double)b.w2[(size_t)64 * co + kk] * b.f2.s[64]);
    if (b.wp)
      for (int cc = 0; cc < ci; ++cc) d[W36Dust::WPCOL + cc] = (float)((double)b.wp[(size_t)64 * ci + cc] * b.fp.s[64]);
    d[W36Dust::B1] = (float)b.f1.t[64];
    d[W36Dust::B2] = (float)b.bias[64];
    if (a.dust_in) {
      for (int pp = 0; pp < 36; ++pp) d[W36Dust::UIN64 + pp] = (float)U[((size_t)64 * ci + 64) * 36 + pp];
      for (int cg = 0; cg < 4; ++cg)
        for (int pp = 0; pp < 36; ++pp)
          for (int n16 = 0; n16 < 16; ++n16)
            d[W36Dust::UIN + (cg * 36 + pp) * 16 + n16] = (float)U[((size_t)(16 * cg + n16) * ci + 64) * 36 + pp];
    }
    for (int ch = 0; ch < a.nchunk; ++ch)
      for (int pp = 0; pp < 36; ++pp)
        for (int kk = 0; kk < 16; ++kk)
          d[W36Dust::UOUT + (ch * 36 + pp) * 16 + kk] = 16 * ch + kk < ci ? (float)U[((size_t)64 * ci + 16 * ch + kk) * 36 + pp] : 0.f;
  }
  return FPC_OK;
}

// OP_BF16: a block, or the transposed convolution (one launch or one parity phase), on bf16 / split operands
static int pack_fblock(const Packer& pk, const Op& op, const fpc_ctx::ConvW& cw) {
  const FKindInfo& k = g_fkinds[op.fkind];
  const BlockBfArgs& a = op.fargs;
  const std::string& p = op.prefix;
  const int ci = op.cin, co = op.cout, nbt = k.WN * k.NB;
  if (op.phase >= 0) {  // ConvTranspose
    const float* w = pk.need("descriptor.up_sample.weight", {256, 128, 3, 3});
    const float* bct = pk.need("descriptor.up_sample.bias", {128});
    Fold f;
    if (!w || !bct || !fold_bn(pk.m, "descriptor.bn", 128, &f, pk.missing)) return FPC_E_MISSING_KEY;
    if (op.phase == 4) {   // convt_bf16_kernel: all nine taps per step of 16 channels, in ConvTTaps' order
      PackSource s{ci, ci, 9,
                   [&](int n, int cc, int t) { return (double)w[((cc * 128 + n) * 3 + ConvTTaps::ky(t)) * 3 + ConvTTaps::kx(t)]; },
                   &f.s};
      if (int rc = pk.put(op, pack_conv_bf16({s}, co, k.CMIDP / 32, 16, 1, &pk.range_bad), cw.w[0])) return rc;
    } else {
      const std::vector<ConvTTap> taps = convt_phase_taps(op.phase);
      PackSource s{ci, a.nchunk * k.KC, (int)taps.size(),
                   [&](int n, int cc, int t) { return (double)w[((cc * 128 + n) * 3 + taps[t].ky) * 3 + taps[t].kx]; },
                   &f.s};
      if (int rc = pk.put(op, pack_conv_bf16({s}, co, nbt, k.KC, k.planes, &pk.range_bad), cw.w[0])) return rc;
    }
    return pk.fill(op, cw.b, co, [&](int n) { return (double)bct[n] * f.s[n] + f.t[n]; });
  }
  BlockWeights b;
  if (!load_block(pk, p, ci, co, a.k16_x > 0, &b)) return FPC_E_MISSING_KEY;
  const bool sc_in_w1 = k.planes == 1;   // (as add_fblock laid the regions out)
  const std::vector<double> ones(co, 1.0);
  // taps 0..8: conv1 x bn1's scale; tap 9 (FPC_BF16): the shortcut on the same channels -- the projection x its bn's
  // scale, or the unit matrix
  PackSource s1{ci, a.nchunk * k.KC, sc_in_w1 ? 10 : 9,
                [&](int n, int c_, int t) {
                  if (t < 9) return (double)b.w1[((size_t)(n * ci + c_)) * 9 + t] * b.f1.s[n];
                  return b.wp ? (double)b.wp[(size_t)n * ci + c_] * b.fp.s[n] : (n == c_ ? 1.0 : 0.0);
                },
                &ones};
  if (int rc = pk.put(op, pack_conv_bf16({s1}, co, nbt, k.KC, k.planes, &pk.range_bad), cw.w[0])) return rc;
  if (int rc = pk.fill(op, cw.b, co, [&](int n) { return b.f1.t[n]; })) return rc;
  if (int rc = pk.put(op, pack_conv_bf16(block_1x1_sources(b, ci, co, a.k16_h * 16, sc_in_w1 ? 0 : a.k16_x * 16), co, nbt, 16, k.planes, &pk.range_bad),
                      cw.w[1]))
    return rc;
  return pk.fill(op, cw.b2, co, [&](int n) { return b.bias[n]; });
}

static int pack_block(const Packer& pk, const Op& op, const fpc_ctx::ConvW& cw) {
  const BKindInfo& k = g_bkinds[op.bkind];
  const BlockArgs& a = op.bargs;
  const int ci = op.cin, co = op.cout, nbt = k.WN * k.NB;
  BlockWeights b;
  if (!load_block(pk, op.prefix, ci, co, a.k8_x > 0, &b)) return FPC_E_MISSING_KEY;
  PackSource s1{ci, a.nchunk * k.KC, 9, [&](int n, int c_, int t) { return (double)b.w1[((size_t)(n * ci + c_)) * 9 + t]; }, &b.f1.s};
  if (int rc = pk.put(op, pack_conv({s1}, co, nbt, k.KC), cw.w[0])) return rc;
  if (int rc = pk.fill(op, cw.b, co, [&](int n) { return b.f1.t[n]; })) return rc;
  if (int rc = pk.put(op, pack_conv(block_1x1_sources(b, ci, co, a.k8_h * 8, a.k8_x * 8), co, nbt, 8), cw.w[1])) return rc;
  return pk.fill(op, cw.b2, co, [&](int n) { return b.bias[n]; });
}

// OP_CONV of the Python network: one half of an unfused block, the detector's separate shortcut, or the transposed
// convolution -- the checkpoint prefix and the role are recovered from the op name
static int pack_conv_op(const Packer& pk, const Op& op, const fpc_ctx::ConvW& cw) {
  const TensorMap& m = pk.m;
  std::string* missing = pk.missing;
  const KindInfo& k = g_kinds[op.kind];
  const ConvArgs& a = op.args;
  const std::string& nm = op.name;
  const size_t dot = nm.find(".conv1+");
  const size_t dot2 = nm.find(".conv2+");
  const int cin0p = a.nchunk0 * k.KC, cin1p = a.nchunk1 * k.KC;
  Fold f, fp;
  std::vector<double> bias(a.nbt * 32, 0.0);
  if (nm == "descriptor.up_sample+bn+relu") {
    const float* w = pk.need("descriptor.up_sample.weight", {256, 128, 3, 3});
    const float* bct = pk.need("descriptor.up_sample.bias", {128});
    if (!w || !bct || !fold_bn(m, "descriptor.bn", 128, &f, missing)) return FPC_E_MISSING_KEY;
    for (int ph = 0; ph < 4; ++ph) {
      const std::vector<ConvTTap> taps = convt_phase_taps(ph);
      PackSource s{256, cin0p, (int)taps.size(),
                   [&](int n, int ci, int t) { return (double)w[((ci * 128 + n) * 3 + taps[t].ky) * 3 + taps[t].kx]; },
                   &f.s};
      if (int rc = pk.put(op, pack_conv({s}, 128, a.nbt, k.KC), cw.w[ph])) return rc;
    }
    for (int n = 0; n < 128; ++n) bias[n] = (double)bct[n] * f.s[n] + f.t[n];
  } else if (nm == "detector.layer.0.identity_downsample") {
    const float* w = pk.need("detector.layer.0.identity_downsample.0.weight", {65, 128, 1, 1});
    if (!w || !fold_bn(m, "detector.layer.0.identity_downsample.1", 65, &f, missing)) return FPC_E_MISSING_KEY;
    PackSource s{128, cin0p, 1, [&](int n, int ci, int) { return (double)w[n * 128 + ci]; }, &f.s};
    if (int rc = pk.put(op, pack_conv({s}, 65, a.nbt, k.KC), cw.w[0])) return rc;
    for (int n = 0; n < 65; ++n) bias[n] = f.t[n];
  } else if (dot != std::string::npos) {  // 3x3 conv1 + bn1
    const std::string p = nm.substr(0, dot);
    auto it = m.find(p + ".conv1.weight");
    if (it == m.end() || it->second.shape.size() != 4 || it->second.shape[2] != 3) {
      if (missing->empty()) *missing = p + ".conv1.weight";
      return FPC_E_MISSING_KEY;
    }
    const int co = (int)it->second.shape[0], ci = (int)it->second.shape[1];
    const float* w = it->second.data;
    if (ci > cin0p || co > a.nbt * 32 || !w) {
      *missing = p + ".conv1.weight";
      return FPC_E_MISSING_KEY;
    }
    if (!fold_bn(m, p + ".bn1", co, &f, missing)) return FPC_E_MISSING_KEY;
    PackSource s{ci, cin0p, 9, [&](int n, int c_, int t) { return (double)w[((size_t)(n * ci + c_)) * 9 + t]; }, &f.s};
    if (int rc = pk.put(op, pack_conv({s}, co, a.nbt, k.KC), cw.w[0])) return rc;
    for (int n = 0; n < co; ++n) bias[n] = f.t[n];
  } else if (dot2 != std::string::npos) {  // 1x1 conv2 + bn2 (+ projection shortcut as a second K source)
    const std::string p = nm.substr(0, dot2);
    auto it = m.find(p + ".conv2.weight");
    if (it == m.end() || it->second.shape.size() != 4 || !it->second.data) {
      if (missing->empty()) *missing = p + ".conv2.weight";
      return FPC_E_MISSING_KEY;
    }
    const int co = (int)it->second.shape[0];
    const float* w = it->second.data;
    if ((int)it->second.shape[1] != co || co > cin0p || co > a.nbt * 32) {
      *missing = p + ".conv2.weight";
      return FPC_E_MISSING_KEY;
    }
    if (!fold_bn(m, p + ".bn2", co, &f, missing)) return FPC_E_MISSING_KEY;
    std::vector<PackSource> srcs;
    srcs.push_back({co, cin0p, 1, [&, co](int n, int c_, int) { return (double)w[(size_t)n * co + c_]; }, &f.s});
    for (int n = 0; n < co; ++n) bias[n] = f.t[n];
    const float* wp = nullptr;
    int cip = 0;
    if (a.in1) {
      auto ip = m.find(p + ".identity_downsample.0.weight");
      if (ip == m.end() || ip->second.shape.size() != 4 || (int)ip->second.shape[0] != co || !ip->second.data ||
          (int)ip->second.shape[1] > cin1p) {
        if (missing->empty()) *missing = p + ".identity_downsample.0.weight";
        return FPC_E_MISSING_KEY;
      }
      wp = ip->second.data;
      cip = (int)ip->second.shape[1];
      if (!fold_bn(m, p + ".identity_downsample.1", co, &fp, missing)) return FPC_E_MISSING_KEY;
      srcs.push_back({cip, cin1p, 1, [&, cip](int n, int c_, int) { return (double)wp[(size_t)n * cip + c_]; }, &fp.s});
      for (int n = 0; n < co; ++n) bias[n] += fp.t[n];
    }
    if (int rc = pk.put(op, pack_conv(srcs, co, a.nbt, k.KC), cw.w[0])) return rc;
  } else {
    *missing = "internal: unknown op " + nm;
    return FPC_E_INVALID;
  }
  return pk.fill(op, cw.b, a.nbt * 32, [&](int n) { return bias[n]; });
}

static int pack_all_impl(fpc_ctx* c, const TensorMap& m, std::string* missing, bool& range_bad) {
  c->host_blob.assign(c->blob_floats, 0.f);
  const Packer pk{c, m, missing, range_bad};
  if (int rc = c->vgg ? pack_vgg_convs(pk) : pack_stem(pk)) return rc;
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    if (c->vgg && op.type != OP_WBLOCK) continue;  // packed above
    int rc = FPC_OK;
    switch (op.type) {
      case OP_WBLOCK: rc = pack_wblock(pk, op, c->convw[i]); break;
      case OP_BF16: rc = pack_fblock(pk, op, c->convw[i]); break;
      case OP_BLOCK: rc = pack_block(pk, op, c->convw[i]); break;
      case OP_CONV: rc = pack_conv_op(pk, op, c->convw[i]); break;
      default: break;
    }
    if (rc != FPC_OK) return rc;
  }
  return FPC_OK;
}

// ---- execution -------------------------------------------------------------------------------
// A call's frames are split into sub-batches that run the whole launch sequence on separate
// HIP streams: workgroups of one sub-batch fill the CUs another leaves idle in the tail of each
// (short) launch, and the latency-bound NMS of one overlaps the MFMA-bound convolutions of the
// other.  Frames are independent, so sub-batches share nothing but the weights.
static hipEvent_t next_event(fpc_ctx* c) {
  if (c->events_used == c->event_pool.size()) {
    hipEvent_t e;
    hipEventCreate(&e);
    c->event_pool.push_back(e);
  }
  return c->event_pool[c->events_used++];
}

struct Sub {
  int f0, n;
  bool small = false;              // the whole call is a few frames: the latency plan (heads side by side, fused layer_in.1)
  bool fuse_softmax = false;       // run_network(which = 1): the detector's last block also does exp-softmax / depth-to-space / threshold
  hipStream_t st;                  // encoder, descriptor head, descriptor sampling
  hipStream_t side = nullptr;      // detector head + NMS, concurrent with the descriptor head
  hipEvent_t ev_enc = nullptr, ev_det = nullptr;
};

struct LaunchTimer {
  fpc_ctx* c;
  int op;
  hipStream_t st;
  int frames;
  hipEvent_t s{}, e{};
  int wkind = -1;
  double mfma_flops = -1.0;
  LaunchTimer(fpc_ctx* c_, int op_, hipStream_t st_, int frames_) : c(c_), op(op_), st(st_), frames(frames_) {
    if (c->timing) {
      s = next_event(c);
      e = next_event(c);
      hipEventRecord(s, st);
    }
  }
  ~LaunchTimer() {
    if (c->timing) {
      hipEventRecord(e, st);
      c->timings.push_back({s, e, op, frames, wkind, mfma_flops});
    }
  }
};

static int op_index(const fpc_ctx* c, OpType t) {
  for (size_t i = 0; i < c->ops.size(); ++i)
    if (c->ops[i].type == t) return (int)i;
  return -1;
}

// which: 0 = encoder, 1 = detector head, 2 = descriptor head
// The diagnostic build's in-kernel stamps for the launch FPC_STAMP_OP names (a no-op in the product library)
template <typename Args>
static void diag_stamp(fpc_ctx* c, const Op& op, Args& a, int tiles) {
#ifdef FPC_DIAG
  a.stamps = nullptr;
  if (const char* e = getenv("FPC_STAMP_OP"))
    if (op.name.find(e) != std::string::npos) {
      if (!c->diag_stamps) hipHostMalloc((void**)&c->diag_stamps, (size_t)65536 * 8 * sizeof(unsigned long long));
      memset(c->diag_stamps, 0, (size_t)65536 * 8 * sizeof(unsigned long long));
      a.stamps = c->diag_stamps;
      c->diag_n = tiles;
    }
#endif
}

// The stem's kernel: chosen HERE, for the launch and for the name fpc_get_timings reports alike
enum StemKind { STEM_PLAIN, STEM_POOL, STEM_POOL2, STEM_X3, STEM_X3_F16, STEM_BF16 };
static StemKind stem_kind(const fpc_ctx* c) {
  if (!(c->opt.fuse_stem_pool || c->cin == 1 || c->bf16)) return STEM_PLAIN;   // conv1 alone: OP_POOL follows
  if (c->split_f16) return STEM_X3_F16;
  if (c->bf16) return STEM_BF16;   // bf16 operands like every other layer of the mode, bf16 out, no atomics
  if (c->split) return STEM_X3;
  return c->opt.stem2 ? STEM_POOL2 : STEM_POOL;
}

// Launches the stem for `sb`'s frames -- unless `sb` is null: the name alone -- and returns its symbol
static const char* launch_stem(fpc_ctx* c, const Op& op, int i, const float* frames, const Sub* sb) {
  static const char* const symbol[] = {"stem_kernel", "stem_pool_kernel", "stem_pool2_kernel", "stem_pool_x3_kernel",
                                       "stem_pool_x3_kernel", "stem_bf16_kernel"};
  const StemKind kind = stem_kind(c);
  if (!sb) return symbol[kind];
  const int H = c->H, W = c->W, n = sb->n, f0 = sb->f0;
  const bool gray = c->cin == 1;
  if (kind == STEM_PLAIN) {
    LaunchTimer t(c, i, sb->st, n);
    StemArgs a = c->stem;
    a.in = frames + (size_t)f0 * 3 * H * W;
    a.out = c->stem_out + (size_t)f0 * (H / 2) * (W / 2) * 64;
    hipLaunchKernelGGL(stem_kernel, dim3(a.tiles_x * a.tiles_y * n), dim3(256), 0, sb->st, a);
    return symbol[kind];
  }
  // the pooled map: fp32, completed across tiles with atomicMax (hence zero-filled); FPC_BF16 writes it once, as bf16
  float* x0 = c->bf16 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(c->x0) + (size_t)f0 * (H / 4) * (W / 4) * 64)
                      : c->x0 + (size_t)f0 * (H / 4) * (W / 4) * 64;
  // (only the cells that tiles complete for each other with atomicMax need the zero: kernels_misc.h)
  if (!c->bf16) stem_border_clear_kernel<<<(n * (H / 4) + 7) / 8, 256, 0, sb->st>>>(reinterpret_cast<float4*>(x0), H / 4, W / 4, n * (H / 4));
  LaunchTimer t(c, i, sb->st, n);
  StemPoolArgs a{};
  a.in = frames + (size_t)f0 * c->cin * H * W;
  a.wfrag = c->stem.wfrag;
  a.bias = c->stem.bias;
  a.out = x0;
  a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2; a.Hp = H / 4; a.Wp = W / 4;
  a.tiles_x = c->stem.tiles_x; a.tiles_y = c->stem.tiles_y;
  a.range = c->range + (size_t)f0 * FPC_RANGE_WORDS;
  const dim3 grid(a.tiles_x * a.tiles_y * n);
  if (kind == STEM_X3 || kind == STEM_X3_F16 || kind == STEM_BF16) {
    StemX3Args x{};
    x.in = a.in; x.wfrag = reinterpret_cast<const uint4*>(a.wfrag); x.bias = a.bias; x.out = a.out;
    x.H = H; x.W = W; x.Ho = a.Ho; x.Wo = a.Wo; x.Hp = a.Hp; x.Wp = a.Wp; x.tiles_x = a.tiles_x; x.tiles_y = a.tiles_y;
    x.range_flag = c->split_f16 ? c->status + 1 : nullptr;
    diag_stamp(c, op, x, a.tiles_x * a.tiles_y * n);
    if (kind == STEM_X3_F16) {
      if (gray) hipLaunchKernelGGL((stem_pool_x3_kernel<1, 2>), grid, dim3(256), 0, sb->st, x);
      else hipLaunchKernelGGL((stem_pool_x3_kernel<3, 2>), grid, dim3(256), 0, sb->st, x);
    } else if (kind == STEM_BF16) {
      x.frames = n;
      x.tiles_x = (x.Wp + SB2_PW - 1) / SB2_PW;   // stem_bf16.h: 8 x 7 pooled pixels per tile
      x.tiles_y = (x.Hp + SB2_PH - 1) / SB2_PH;
      const int T = x.tiles_x * x.tiles_y * n;
      const dim3 pg(bf16_persistent_grid(T, 2 * c->num_cus, 1, c->opt.bf16_grid));  // two workgroups per CU, a multiple of 8
      if (gray) hipLaunchKernelGGL(stem_bf16_kernel<1>, pg, dim3(SB2_THREADS), StemB2Cfg<1>::LDS_BYTES, sb->st, x);
      else hipLaunchKernelGGL(stem_bf16_kernel<3>, pg, dim3(SB2_THREADS), StemB2Cfg<3>::LDS_BYTES, sb->st, x);
    } else {
      if (gray) hipLaunchKernelGGL((stem_pool_x3_kernel<1, 3>), grid, dim3(256), 0, sb->st, x);
      else hipLaunchKernelGGL((stem_pool_x3_kernel<3, 3>), grid, dim3(256), 0, sb->st, x);
    }
    return symbol[kind];
  }
  if (kind == STEM_POOL2) {
    if (gray) hipLaunchKernelGGL(stem_pool2_kernel<1>, grid, dim3(256), 0, sb->st, a);
    else hipLaunchKernelGGL(stem_pool2_kernel<3>, grid, dim3(256), 0, sb->st, a);
  } else {
    if (gray) hipLaunchKernelGGL(stem_pool_kernel<1>, grid, dim3(256), 0, sb->st, a);
    else hipLaunchKernelGGL(stem_pool_kernel<3>, grid, dim3(256), 0, sb->st, a);
  }
  return symbol[kind];
}

static void launch_pool(fpc_ctx* c, int i, const Sub& sb) {
  if (stem_kind(c) != STEM_PLAIN) return;   // the stem pooled its own map
  const int H = c->H, W = c->W, n = sb.n, f0 = sb.f0;
  LaunchTimer t(c, i, sb.st, n);
  const size_t total = (size_t)n * (H / 4) * (W / 4) * 16;
  hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, sb.st,
                     reinterpret_cast<const float4*>(c->stem_out + (size_t)f0 * (H / 2) * (W / 2) * 64),
                     reinterpret_cast<float4*>(c->x0 + (size_t)f0 * (H / 4) * (W / 4) * 64), n, H / 2, W / 2, H / 4, W / 4);
}

static void launch_wblock(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  const int n = sb.n, f0 = sb.f0;
  LaunchTimer t(c, i, sb.st, n);
  WBlockArgs a = op.wargs;
  a.frame0 = f0;
  diag_stamp(c, op, a, a.tiles_x * a.tiles_y * n);
  a.total = a.tiles_x * a.tiles_y * n;
  a.xcd_order = c->opt.xcd_order ? 1 : 0;
  {  // range of the input's buffer descriptor: frames 0 .. f0 + n - 1 of the tensor, from `x` (already offset to its first channel)
    const unsigned long long xb = (unsigned long long)(f0 + n) * a.H * a.W * a.csx * sizeof(float);
    a.x_bytes = xb > W16_REACH ? (unsigned)W16_REACH : (unsigned)xb;
  }
  // persistent (one workgroup per CU walking the tiles) when a workgroup gets enough tiles to
  // amortise; otherwise one workgroup per tile
  int grid = (c->opt.persist_min_tiles > 0 && a.total >= c->opt.persist_min_tiles * c->num_cus) ? c->num_cus : a.total;
  if (g_wkinds[op.wkind].gen == 3) {
    // Pointers to the launch's first frame, as many frames per launch as stay below W36_MARKER bytes (all of them,
    // except at the C++ network's full-resolution layers: 78.6 MB per VGA frame and tensor).
    const int fpl = w36_frames_per_launch(a.H, a.W, a.csx, a.cso);
    const float* x0 = a.x;
    float* o0 = a.out;
    const int Hf = a.H, tx_f = a.tiles_x, ty_f = a.tiles_y;
    const WKind sk = c->opt.tiles_round6 ? w36_stacked_kind(op.wkind) : WK_COUNT;
    double mf = 0.0;
    for (int g0 = 0; g0 < n; g0 += fpl) {
      const int gn = std::min(fpl, n - g0);
      a.frame0 = 0;
      a.x = x0 + (size_t)(f0 + g0) * Hf * a.W * a.csx;
      a.out = o0 + (size_t)(f0 + g0) * Hf * a.W * a.cso;
      a.x_bytes = (unsigned)((unsigned long long)gn * Hf * a.W * a.csx * sizeof(float));
      // round 6: the launch's frames as ONE image of gn x Hf rows where that is fewer tiles (wblock36s_kernel)
      const int srows = w36_stacked_rows(Hf, a.W, gn, sk, tx_f * ty_f);
      const WKind lk = srows ? sk : op.wkind;
      a.H = srows ? gn * Hf : Hf;
      a.frame_h = srows ? Hf : 0;
      a.tiles_x = srows ? (a.W + g_wkinds[sk].TW - 1) / g_wkinds[sk].TW : tx_f;
      a.tiles_y = srows ? srows : ty_f;
      a.total = srows ? a.tiles_x * srows : tx_f * ty_f * gn;
      if (srows) t.wkind = sk;
      mf += srows ? wkind_mfma_flops(g_wkinds[sk], a.total, a.nchunk, a.k8_h + a.k8_x) : op.mfma_flops_per_frame * gn;
      // One workgroup per CU (137 KB of LDS), so a launch lasts ceil(tiles / CUs) tile times whatever the grid: take
      // the SMALLEST grid that still finishes in that many rounds (a multiple of 8: the tile walk is per XCD) and
      // leave the other CUs to the launches of the other sub-batch's stream -- 640 tiles: 216 workgroups x 3 rounds
      // instead of 256 of which 128 idle through the third; 320 tiles: 160 x 2.
      // (a launch of gridDim.y parts shares the CUs between them: each part's tile walk gets CUs / parts)
      const int cus_cap = c->opt.w36_cus > 0 ? std::min(c->num_cus, c->opt.w36_cus) : c->num_cus;
      const int cus8 = std::max(1, cus_cap / 8 / std::max(1, op.grid_y)), per_xcd = (a.total + 7) / 8;
      const int rounds = (per_xcd + cus8 - 1) / cus8;
      const int grid3 = 8 * std::min(cus8, (per_xcd + rounds - 1) / rounds);
      g_wkinds[lk].launch(a, dim3(std::min(a.total, grid3), op.grid_y), sb.st);
    }
    if (t.wkind >= 0) t.mfma_flops = mf;
    return;
  }
  g_wkinds[op.wkind].launch(a, dim3(std::min(a.total, grid), op.grid_y), sb.st);
}

static void launch_block(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  LaunchTimer t(c, i, sb.st, sb.n);
  BlockArgs a = op.bargs;
  a.frame0 = sb.f0;
  diag_stamp(c, op, a, a.tiles_x * a.tiles_y * sb.n);
  g_bkinds[op.bkind].launch(a, dim3(a.tiles_x * a.tiles_y * sb.n), sb.st);
}

static void launch_fblock(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  const int n = sb.n, f0 = sb.f0;
  LaunchTimer t(c, i, sb.st, n);
  BlockBfArgs a = op.fargs;
  a.frame0 = f0;
  a.range_flag = c->split_f16 ? c->status + 1 : nullptr;
  diag_stamp(c, op, a, a.tiles_x * a.tiles_y * n);
  if (g_fkinds[op.fkind].planes != 1) {
    g_fkinds[op.fkind].launch(a, dim3(a.tiles_x * a.tiles_y * n), sb.st);
    return;
  }
  // block_bf16_kernel: persistent grid, a multiple of 8 (block_bf16.h)
  a.total_tiles = a.tiles_x * a.tiles_y * n;
  if (sb.fuse_softmax && op.fused_softmax_capable) {
    const size_t HW = (size_t)c->H * c->W;
    hipMemsetAsync(c->ncand + f0, 0, sizeof(int32_t) * n, sb.st);
    a.softmax = 1;
    a.thresh = c->cfg.conf_thresh;
    a.nmsmap = c->nmsmap + f0 * HW;
    a.cand = c->cand + f0 * HW;
    a.ncand = c->ncand + f0;
  }
  // (op.grid_y parts -- convt_bf16_kernel's output-channel halves -- share the CUs)
  const int g = bf16_persistent_grid(a.total_tiles, c->fkind_blocks_per_cu[op.fkind] * c->num_cus, op.grid_y, c->opt.bf16_grid);
  g_fkinds[op.fkind].launch(a, dim3(g, op.grid_y), sb.st);
}

static void launch_conv(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  LaunchTimer t(c, i, sb.st, sb.n);
  ConvArgs a = op.args;
  a.frame0 = sb.f0;
  const dim3 grid(a.tiles_x * a.tiles_y * sb.n, op.grid_y, op.grid_z);
  if (op.lean) lean_kind(op.kind)->launch(a, grid, sb.st);
  else g_kinds[op.kind].launch(a, grid, sb.st);
}

// The C++ network's own layers: its first convolution, its max-pools, the descriptor normalisation
static void launch_vconv0(fpc_ctx* c, const Op& op, int i, const float* frames, const Sub& sb) {
  LaunchTimer t(c, i, sb.st, sb.n);
  VggConv0Args a{};
  a.in = frames;
  a.w = c->blob + c->vconv0_off;
  a.out = op.pout;
  a.H = c->H; a.W = c->W; a.frame0 = sb.f0;
  hipLaunchKernelGGL(vgg_conv0_kernel, dim3((unsigned)((size_t)sb.n * c->H * c->W / 64)), dim3(256), 0, sb.st, a);
}
static void launch_pool2(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  LaunchTimer t(c, i, sb.st, sb.n);
  const size_t tot = (size_t)sb.n * (op.pH / 2) * (op.pW / 2) * (op.pC / 4);
  hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, sb.st,
                     reinterpret_cast<const float4*>(op.pin), reinterpret_cast<float4*>(op.pout), sb.n, op.pH, op.pW,
                     op.pC / 4, sb.f0);
}
static void launch_l2norm(fpc_ctx* c, const Op& op, int i, const Sub& sb) {
  LaunchTimer t(c, i, sb.st, sb.n);
  const size_t npix = (size_t)sb.n * c->Hc * c->Wc;
  hipLaunchKernelGGL(l2norm256_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, sb.st,
                     op.pout + (size_t)sb.f0 * c->Hc * c->Wc * 256, npix);
}

// which: 0 = encoder, 1 = detector head, 2 = descriptor head
static void run_network(fpc_ctx* c, const float* frames, const Sub& sb0, int which, hipStream_t st) {
  Sub sb = sb0;
  sb.st = st;
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    const int br = op.descriptor_branch ? 2 : (op.name.compare(0, 8, "detector") == 0 ? 1 : 0);
    if (br != which) continue;
    if (op.shadow) continue;
    if (op.when == 1 && !sb.small) continue;   // variants of a layer for small / large calls
    if (op.when == 2 && sb.small) continue;
    switch (op.type) {
      case OP_STEM: launch_stem(c, op, (int)i, frames, &sb); break;
      case OP_POOL: launch_pool(c, (int)i, sb); break;
      case OP_WBLOCK: launch_wblock(c, op, (int)i, sb); break;
      case OP_BLOCK: launch_block(c, op, (int)i, sb); break;
      case OP_BF16: launch_fblock(c, op, (int)i, sb); break;
      case OP_CONV: launch_conv(c, op, (int)i, sb); break;
      case OP_VCONV0: launch_vconv0(c, op, (int)i, frames, sb); break;
      case OP_POOL2: launch_pool2(c, op, (int)i, sb); break;
      case OP_L2NORM: launch_l2norm(c, op, (int)i, sb); break;
      default: break;  // post-processing ops are issued by the callers
    }
  }
}

static Sub on(const Sub& sb, hipStream_t st) {
  Sub r = sb;
  r.st = st;
  return r;
}

static void run_softmax(fpc_ctx* c, const Sub& sb, bool dense_map = true) {
  const size_t HW = (size_t)c->H * c->W;
  hipMemsetAsync(c->ncand + sb.f0, 0, sizeof(int32_t) * sb.n, sb.st);
  LaunchTimer t(c, op_index(c, OP_SOFTMAX), sb.st, sb.n);
  // (FPC_BF16: the arithmetic of that mode's fused epilogue -- v_exp_f32, one reciprocal per cell; nms_word.h)
  const auto kern = c->bf16 ? softmax_d2s_kernel<true> : softmax_d2s_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(sb.n * c->Hc), dim3(256), (size_t)12 * c->W * sizeof(float), sb.st,
                     c->lg + (size_t)sb.f0 * c->Hc * c->Wc * c->lgcs, c->lgcs, sb.n, c->Hc, c->Wc, c->cfg.conf_thresh,
                     dense_map ? c->prob + sb.f0 * HW : nullptr, c->nmsmap + sb.f0 * HW, c->cand + sb.f0 * HW, c->ncand + sb.f0,
                     c->rowmax + (size_t)sb.f0 * c->Hc);
}

static void run_nms(fpc_ctx* c, const Sub& sb) {
  LaunchTimer t(c, op_index(c, OP_NMS), sb.st, sb.n);
  const size_t HW = (size_t)c->H * c->W;
  const int n = sb.n, f0 = sb.f0;
  NmsArgs a{};
  a.nmsmap = c->nmsmap + f0 * HW; a.cand = c->cand + f0 * HW; a.ncand = c->ncand + f0;
  a.sort_scratch = c->sort_scratch + (size_t)f0 * c->sort_cap;
  a.sort_cap = c->sort_cap;
  const bool chunked = !c->opt.nms_one_workgroup;
  a.aux = chunked ? c->nms_aux + (size_t)f0 * NMS_AUX_INTS : nullptr;
  a.H = c->H; a.W = c->W; a.r = c->cfg.nms_dist; a.border = c->cfg.border_remove; a.cap = c->cap;
  a.count = c->count + f0; a.xy = c->xy + (size_t)f0 * c->cap * 2; a.conf = c->conf + (size_t)f0 * c->cap;
  a.status = c->status;
  a.max_rounds = c->H * c->W;
  // enough workgroups that a typical frame (a few thousand candidates) has about one candidate
  // per thread; the second launch normally finds nothing left to do
  const int G = c->opt.nms_g > 0 ? c->opt.nms_g : std::max(1, std::min(16, 512 / n));
  for (int pass = 0; pass < c->opt.nms_passes; ++pass) {
    if (c->cfg.nms_dist == 4)
      hipLaunchKernelGGL(nms_rounds_kernel<4>, dim3(G, n), dim3(NMS_ROUNDS_THREADS), 0, sb.st, a);
    else
      hipLaunchKernelGGL(nms_rounds_kernel<0>, dim3(G, n), dim3(NMS_ROUNDS_THREADS), 0, sb.st, a);
  }
  if (chunked) {
    // the leftovers of the round launches settled by one workgroup per frame, then slices of the candidate list sorted
    // by one workgroup each and merged by rank (kernels_misc.h); nms_sort_kernel leaves at once unless a slice had
    // more survivors than LDS holds
    const bool big = HW > 400000;
    const int GC = big ? 8 : 4;  // a frame of a few thousand candidates has this many slices
    hipLaunchKernelGGL(nms_finish_kernel, dim3(n), dim3(NMS_FINISH_THREADS), 0, sb.st, a);
    if (big) {
      hipLaunchKernelGGL(nms_chunk_sort_kernel<4096>, dim3(GC, n), dim3(1024), 4096 * sizeof(unsigned long long), sb.st, a);
      hipLaunchKernelGGL(nms_merge_kernel<4096>, dim3(GC, n), dim3(1024), 4096 * sizeof(unsigned long long), sb.st, a);
    } else {
      hipLaunchKernelGGL(nms_chunk_sort_kernel<2048>, dim3(GC, n), dim3(1024), 2048 * sizeof(unsigned long long), sb.st, a);
      hipLaunchKernelGGL(nms_merge_kernel<2048>, dim3(GC, n), dim3(1024), 2048 * sizeof(unsigned long long), sb.st, a);
    }
  }
  hipLaunchKernelGGL(nms_sort_kernel, dim3(n), dim3(1024), chunked ? 0 : NMS_LDS_KEYS * sizeof(unsigned long long), sb.st, a);
}

static void run_desc(fpc_ctx* c, const Sub& sb, const float* dmap_nhwc) {
  LaunchTimer t(c, op_index(c, OP_DESC), sb.st, sb.n);
  // persistent grid, a multiple of 8 (kernels_misc.h): eight workgroups of four waves per CU
  const int by_xcd = sb.n >= 8;
  const int G = std::max(8, c->num_cus * 8 / 8 * 8);
  if (c->D == 256)
    hipLaunchKernelGGL(descriptor16_kernel<16>, dim3(G), dim3(256), 0, sb.st,
                       dmap_nhwc + (size_t)sb.f0 * c->Hc * c->Wc * 256, 256, c->Hc, c->Wc, c->H, c->W, c->count + sb.f0,
                       c->xy + (size_t)sb.f0 * c->cap * 2, c->cap, c->desc_out + (size_t)sb.f0 * c->cap * 256, sb.n, by_xcd);
  else if (c->bf16 && dmap_nhwc == c->desc_map)   // FPC_BF16's own map is bf16: half the elements' bytes per frame
    hipLaunchKernelGGL((descriptor16_kernel<8, true>), dim3(G), dim3(256), 0, sb.st,
                       reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(dmap_nhwc) + (size_t)sb.f0 * c->Hc * c->Wc * 128),
                       128, c->Hc, c->Wc, c->H, c->W, c->count + sb.f0,
                       c->xy + (size_t)sb.f0 * c->cap * 2, c->cap, c->desc_out + (size_t)sb.f0 * c->cap * 128, sb.n, by_xcd);
  else
    hipLaunchKernelGGL(descriptor16_kernel<8>, dim3(G), dim3(256), 0, sb.st,
                       dmap_nhwc + (size_t)sb.f0 * c->Hc * c->Wc * 128, 128, c->Hc, c->Wc, c->H, c->W, c->count + sb.f0,
                       c->xy + (size_t)sb.f0 * c->cap * 2, c->cap, c->desc_out + (size_t)sb.f0 * c->cap * 128, sb.n, by_xcd);
}

// Splits [0,n) over the ctx's streams; aux streams fork from / join into the main stream.
template <typename F>
static int for_each_sub(fpc_ctx* c, int n, F&& body) {
  // fpc_set_timing(n > 1): every n-th pass over a batch carries the events -- decided HERE, for every entry point alike
  // (fpc_detect, fpc_forward, fpc_detect_u8*, each network pass of fpc_homography_adaptation)
  if (c->timing_every > 1) c->timing = c->timing_calls++ % c->timing_every == 0;
  int parts = std::min<int>((int)c->aux.size() + 1, std::max(1, n / c->opt.min_sub));
  if (parts > 1) HIPCHECK(hipEventRecord(c->ev_fork, c->stream));
  int f0 = 0;
  for (int p = 0; p < parts; ++p) {
    const int cnt = n / parts + (p < n % parts ? 1 : 0);
    Sub sb;
    sb.f0 = f0;
    sb.n = cnt;
    sb.small = n < 2 * c->opt.min_sub && n <= c->small_reach;
    sb.st = p == 0 ? c->stream : c->aux[p - 1];
    sb.side = c->side[p];
    // The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES) in creation order, and two
    // streams on one queue run in order: with main, aux1, aux2, side0 the side stream shared the main stream's queue
    // and a single frame's heads no longer overlapped (0.81 instead of 0.62 ms in the split mode).  A call of a few
    // frames has one sub-batch, so the first aux stream -- created right behind the main stream -- is idle: use it.
    if (sb.small && !c->aux.empty()) sb.side = c->aux[0];
    sb.ev_enc = c->ev_enc[p];
    sb.ev_det = c->ev_det[p];
    if (p) HIPCHECK(hipStreamWaitEvent(sb.st, c->ev_fork, 0));
    body(sb);
    if (p) {
      HIPCHECK(hipEventRecord(c->ev_join[p - 1], sb.st));
      HIPCHECK(hipStreamWaitEvent(c->stream, c->ev_join[p - 1], 0));
    }
    f0 += cnt;
  }
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

// The whole path for one sub-batch.  The detector head and its post-processing (latency-bound,
// few CUs) run on a side stream next to the descriptor head (MFMA-bound); both only need the
// encoder output.  `upto`: 0 = dense maps only (fpc_forward), 1 = keypoints + descriptors.
static void run_path(fpc_ctx* c, const float* frames, const Sub& sb0, bool de, int upto) {
  // fpc_detect in FPC_BF16: the detector's last block writes the NMS state map and the candidate lists itself (the
  // logits and the dense probability map, which only fpc_forward's callers see, are not produced)
  Sub sb = sb0;
  for (const Op& op : c->ops) sb.fuse_softmax |= upto && op.fused_softmax_capable;
  c->logits_valid = !sb.fuse_softmax;
  hipMemsetAsync(c->range + (size_t)sb.f0 * FPC_RANGE_WORDS, 0, sizeof(uint32_t) * FPC_RANGE_WORDS * sb.n, sb.st);
  run_network(c, frames, sb, 0, sb.st);
  if (de && upto && c->opt.nms_aside && !sb.small && sb.side) {
    // detector head and softmax in line; the (latency-bound, few-CU) NMS on the side stream next to the descriptor head
    run_network(c, frames, sb, 1, sb.st);
    if (!sb.fuse_softmax) run_softmax(c, sb, !upto);
    hipEventRecord(sb.ev_enc, sb.st);
    hipStreamWaitEvent(sb.side, sb.ev_enc, 0);
    run_nms(c, on(sb, sb.side));
    hipEventRecord(sb.ev_det, sb.side);
    run_network(c, frames, sb, 2, sb.st);
    hipStreamWaitEvent(sb.st, sb.ev_det, 0);
    run_desc(c, sb, c->desc_map);
    return;
  }
  if (!de || !(c->opt.split_heads || sb.small) || !sb.side) {
    run_network(c, frames, sb, 1, sb.st);
    if (!sb.fuse_softmax) run_softmax(c, sb, !upto);
    if (upto) run_nms(c, sb);
    if (de) {
      run_network(c, frames, sb, 2, sb.st);
      if (upto) run_desc(c, sb, c->desc_map);
    }
    return;
  }
  hipEventRecord(sb.ev_enc, sb.st);
  hipStreamWaitEvent(sb.side, sb.ev_enc, 0);
  const Sub det = on(sb, sb.side);
  run_network(c, frames, sb, 1, sb.side);
  if (!sb.fuse_softmax) run_softmax(c, det, !upto);
  if (upto) run_nms(c, det);
  hipEventRecord(sb.ev_det, sb.side);
  run_network(c, frames, sb, 2, sb.st);
  hipStreamWaitEvent(sb.st, sb.ev_det, 0);
  if (upto) run_desc(c, sb, c->desc_map);
}

}  // namespace fpc

// ====================================================================================
// C-ABI
// ====================================================================================
extern "C" {

int fpc_abi_version(void) { return FPC_ABI_VERSION; }
int fpc_pack_layout_revision(void) { return FPC_PACK_LAYOUT_REVISION; }

// What this binary was compiled with: the target, whether it is the diagnostic build (in-kernel stamps: never the
// product), and that no experiment switch of earlier rounds reached it (they are gone from the headers; a build
// that defines one of their names anyway does not compile).
#if defined(STEMB_SKIP_LOAD) || defined(STEMB_SKIP_K) || defined(STEMB_SKIP_TILE) || defined(STEMB_SKIP_POOL) || \
    defined(STEMB_SKIP_STORE) || defined(W16_YOUNG_PRIO) || defined(W16_PRIO_SPLIT) || defined(FPC_NO_PIN)
#error "ablation switches are not part of the library: see experiments/harness/"
#endif
const char* fpc_build_flags(void) {
  return "arch=gfx950"
#ifdef FPC_DIAG
         ";diag=1"
#else
         ";diag=0"
#endif
         ";ablations=none";
}

const char* fpc_strerror(int code) {
  switch (code) {
    case FPC_OK: return "ok";
    case FPC_E_INVALID: return "invalid argument or unsupported geometry";
    case FPC_E_NO_DEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case FPC_E_HIP: return "HIP runtime error (see fpc_last_hip_error)";
    case FPC_E_NO_WEIGHTS: return "weights not loaded";
    case FPC_E_MISSING_KEY: return "checkpoint entry missing or of the wrong shape (see fpc_last_hip_error)";
    case FPC_E_CAPACITY: return "caller buffer too small";
    case FPC_E_NOT_CONVERGED: return "NMS round limit hit";
    case FPC_E_RANGE: return "value outside fp16's range in FPC_F32_SPLIT_F16 mode (use FPC_F32_SPLIT or FPC_F32)";
    case FPC_E_NONFINITE: return "a frame of the call holds a NaN or Inf pixel (see fpc_last_hip_error for which)";
    default: return "unknown error";
  }
}

const char* fpc_last_hip_error(void) { return g_hip_err.c_str(); }

int fpc_default_config(fpc_config* cfg) {
  if (!cfg) return FPC_E_INVALID;
  memset(cfg, 0, sizeof(*cfg));
  cfg->device = 0;
  cfg->height = 480;
  cfg->width = 640;
  cfg->max_batch = 1;
  cfg->cell = 8;
  cfg->nms_dist = 4;
  cfg->conf_thresh = 0.015f;
  cfg->border_remove = 4;
  cfg->descriptor_enabled = 1;
  cfg->max_keypoints = 0;
  return FPC_OK;
}

// ------------------------------------------------------------------------------------
// Streams on distinct hardware queues: queue_map.h (anchors, device timestamps, a registry of the live contexts' streams)
// ------------------------------------------------------------------------------------
enum { SLOT_MAIN = 0, SLOT_AUX = 1, SLOT_SIDE = 100, SLOT_UPLOAD = 200 };

// Dynamic-LDS limits of every kernel instance and the occupancy table of the bf16 / split-operand instances.
static int prepare_kernels(fpc_ctx* c, const fpc_config* cfg) {
  if (int rc = allow_dynamic_lds(g_kinds)) return rc;
  if (int rc = allow_dynamic_lds(g_lean_kinds)) return rc;
  if (int rc = allow_dynamic_lds(g_wkinds)) return rc;
  if (int rc = allow_dynamic_lds(g_bkinds)) return rc;
  if (int rc = allow_dynamic_lds(g_fkinds)) return rc;
  static_assert(FK_COUNT <= 64, "fpc_ctx::fkind_blocks_per_cu");
  for (int k = 0; k < FK_COUNT; ++k) {
    int nb = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, g_fkinds[k].fn, g_fkinds[k].threads, g_fkinds[k].lds_bytes));
    c->fkind_blocks_per_cu[k] = std::max(1, nb);
  }
  HIPCHECK(hipFuncSetAttribute((const void*)softmax_d2s_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               12 * cfg->width * (int)sizeof(float)));
  HIPCHECK(hipFuncSetAttribute((const void*)softmax_d2s_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               12 * cfg->width * (int)sizeof(float)));
  HIPCHECK(hipFuncSetAttribute((const void*)stem_bf16_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, StemB2Cfg<1>::LDS_BYTES));
  HIPCHECK(hipFuncSetAttribute((const void*)stem_bf16_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, StemB2Cfg<3>::LDS_BYTES));
  HIPCHECK(hipFuncSetAttribute((const void*)nms_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               NMS_LDS_KEYS * (int)sizeof(unsigned long long)));
#ifdef FPC_DIAG
  print_occupancy(g_fkinds);
  print_occupancy(g_bkinds);
  print_occupancy(g_kinds);
#endif
  return FPC_OK;
}

int fpc_create(fpc_ctx** out, const fpc_config* cfg) {
  if (!out || !cfg) return FPC_E_INVALID;
  *out = nullptr;
  // the descriptor head halves the 1/8 map and doubles it again (superpoint.py:43-59): odd
  // H/8 or W/8 breaks its concat, so frames must be multiples of 16 unless it is disabled
  const int mult = (cfg->descriptor_enabled && cfg->arch != FPC_ARCH_VGG) ? 16 : 8;
  if (cfg->in_channels != 0 && cfg->in_channels != 1 && cfg->in_channels != 3) return FPC_E_INVALID;
  if (cfg->dtype < FPC_F32 || cfg->dtype > FPC_F32_SPLIT_F16) return FPC_E_INVALID;
  if (cfg->arch != FPC_ARCH_RESNET && cfg->arch != FPC_ARCH_VGG) return FPC_E_INVALID;
  // the C++ network takes one gray plane (cpp/src/settings.h:19) and has no bf16 plan
  if (cfg->arch == FPC_ARCH_VGG && (cfg->in_channels != 1 || cfg->dtype == FPC_BF16)) return FPC_E_INVALID;
  // conf_thresh: finite and >= 0.  The maps are probabilities (>= 0), so a negative threshold means the same as 0; it
  // is refused rather than silently clamped.  (The reference compares `prob >= thresh` with any float: netutils.py:59.)
  if (!(cfg->conf_thresh >= 0.f) || !(cfg->conf_thresh <= 3.0e38f)) return FPC_E_INVALID;
  if (cfg->cell != 8 || cfg->height < 16 || cfg->width < 16 || cfg->height % mult || cfg->width % mult ||
      cfg->max_batch < 1 || cfg->nms_dist < 0 || cfg->nms_dist > 64 || cfg->border_remove < 0 ||
      (long long)cfg->height * cfg->width >= (1ll << 30) ||
      // the kernels address a tensor of the whole batch with 32-bit byte offsets (the widest: 16 bytes per frame pixel)
      (long long)cfg->max_batch * cfg->height * cfg->width >= (1ll << 28) ||
      cfg->width > 3328)  // softmax_d2s_kernel keeps an 8 x W strip (48 W bytes) in the 160 KB of LDS
    return FPC_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
    g_hip_err = "hipGetDeviceCount: no device";
    return FPC_E_NO_DEVICE;
  }
  HIPCHECK(hipSetDevice(cfg->device));
  std::unique_ptr<fpc_ctx> c(new fpc_ctx());
  {
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, cfg->device));
    c->num_cus = std::max(1, prop.multiProcessorCount);
  }
  c->cfg = *cfg;
  // launch-plan options: plan_flags and the config's fields first, then the FPC_* variables over them (plan_options.h)
  c->opt = resolve_plan_options(*cfg, [](const char* name) -> const char* { return getenv(name); });
  c->H = cfg->height;
  c->W = cfg->width;
  c->B = cfg->max_batch;
  c->Hc = c->H / 8;
  c->Wc = c->W / 8;
  c->cin = cfg->in_channels == 1 ? 1 : 3;
  c->vgg = cfg->arch == FPC_ARCH_VGG;
  c->D = c->vgg ? 256 : 128;
  c->bf16 = cfg->dtype == FPC_BF16;
  c->split = cfg->dtype == FPC_F32_SPLIT || cfg->dtype == FPC_F32_SPLIT_F16;
  c->split_f16 = cfg->dtype == FPC_F32_SPLIT_F16;
  c->lgcs = (c->bf16 || c->split) ? 80 : 72;
  // kept points are pairwise > nms_dist apart (infinity norm): at most one per (r+1)^2 cell
  const int r1 = cfg->nms_dist + 1;
  const int worst = ((c->H + r1 - 1) / r1) * ((c->W + r1 - 1) / r1);
  c->cap = cfg->max_keypoints > 0 ? cfg->max_keypoints : worst;
  c->sort_cap = 1;
  while (c->sort_cap < worst) c->sort_cap <<= 1;
  // Kernel attributes first: the process's first call loads the code object here (~150 ms), so that the stream placement
  // below -- whose first probe launch would otherwise trigger that load -- reports its own cost (fpc_stream_report).
  {
    const int prc = prepare_kernels(c.get(), cfg);
    if (prc != FPC_OK) return prc;      // (nothing to give back yet: no stream, no event, no allocation)
  }
  // Streams: placed on hardware queues of their own (queue_map.h).  The registry's lock is held while this context's
  // streams are chosen and registered, and RELEASED before anything that can fail and call fpc_destroy (round 4 held it
  // to the end of the function: a failing build_plan then deadlocked on fpc_destroy's own lock).
  const bool qprobe = qmap::probe_mode() != 0;
  c->queue_probe = qprobe;
  const auto create_t0 = std::chrono::steady_clock::now();
  std::unique_lock<std::mutex> queue_lock(qmap::state().mu);
  const int probe_rounds0 = qmap::state().dev[cfg->device].rounds;
  c->stream = qmap::acquire(cfg->device, c.get(), SLOT_MAIN, true, qprobe, true);
  if (!c->stream) { qmap::release_owner(c.get()); g_hip_err = "hipStreamCreateWithFlags"; return FPC_E_HIP; }
  c->own_stream = true;
  {
    const int nsub = c->opt.nsub, nside = c->opt.nside;
    // (from here to the end of the stream block: a failure leaves through `fail`, which drops the lock first)
    auto fail = [&](const char* what) {
      g_hip_err = what;
      queue_lock.unlock();
      fpc_destroy(c.release());
      return FPC_E_HIP;
    };
    if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreateWithFlags");
    for (int i = 1; i < nsub; ++i) {
      hipStream_t st = qmap::acquire(cfg->device, c.get(), SLOT_AUX + (i - 1), true, qprobe, true);
      hipEvent_t ev;
      if (!st) return fail("hipStreamCreateWithFlags");
      c->aux.push_back(st);
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreateWithFlags");
      c->ev_join.push_back(ev);
    }
    for (int i = 0; i < nsub; ++i) {
      hipStream_t st = nullptr;
      hipEvent_t e1, e2;
      if (i < nside) {
        st = qmap::acquire(cfg->device, c.get(), SLOT_SIDE + i, false, qprobe, true);
        if (!st) return fail("hipStreamCreateWithFlags");
      }
      c->side.push_back(st);
      if (hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreateWithFlags");
      c->ev_enc.push_back(e1);
      if (hipEventCreateWithFlags(&e2, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreateWithFlags");
      c->ev_det.push_back(e2);
    }
    c->probe_rounds = qmap::state().dev[cfg->device].rounds - probe_rounds0;
    c->placement_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - create_t0).count();
    queue_lock.unlock();
  }
  int rc = FPC_OK;
  // (test hook: the failure path below -- streams, events, registry entries and whatever build_plan had allocated given
  // back, the error code returned -- cannot be reached on this pool's 288 GB otherwise)
  if (rc == FPC_OK && getenv("FPC_TEST_FAIL_CREATE")) {
    g_hip_err = "FPC_TEST_FAIL_CREATE is set: fpc_create's failure path was asked for";
    rc = FPC_E_HIP;
  }
  if (rc == FPC_OK) rc = build_plan(c.get());
  if (rc == FPC_OK && c->plan_error) {
    g_hip_err = "no kernel instance for a layer of this dtype / arch combination";
    rc = FPC_E_INVALID;
  }
  if (rc != FPC_OK) {
    fpc_destroy(c.release());  // streams, events and whatever build_plan had allocated
    return rc;
  }
  *out = c.release();
  return FPC_OK;
}

void fpc_destroy(fpc_ctx* c) {
  if (!c) return;
  hipSetDevice(c->cfg.device);
  hipDeviceSynchronize();
  for (auto e : c->event_pool) hipEventDestroy(e);
  for (auto e : c->ev_join) hipEventDestroy(e);
  for (auto e : c->ev_enc) hipEventDestroy(e);
  for (auto e : c->ev_det) hipEventDestroy(e);
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  {
    // the ctx's own streams (idle: the device was waited for above) go back to the device's spare list with the queue
    // they were found on -- the next fpc_create takes them from there (queue_map.h); a caller's stream is not ours
    std::lock_guard<std::mutex> queue_lock(qmap::state().mu);
    qmap::DeviceQueues& q = qmap::state().dev[c->cfg.device];
    auto give_back = [&](hipStream_t st, int slot) {
      if (!st) return;
      const qmap::Placed* p = qmap::find(c, slot);
      qmap::retire(q, st, p && p->st == st ? p->qclass : qmap::Q_UNKNOWN);
    };
    for (size_t i = 0; i < c->aux.size(); ++i) give_back(c->aux[i], SLOT_AUX + (int)i);
    for (size_t i = 0; i < c->side.size(); ++i) give_back(c->side[i], SLOT_SIDE + (int)i);
    give_back(c->upload, SLOT_UPLOAD);
    if (c->own_stream) give_back(c->stream, SLOT_MAIN);
    qmap::release_owner(c);
  }
  for (Slab* s : c->slabs) s->release();
  if (c->blob) hipFree(c->blob);
  if (c->u8stage) hipFree(c->u8stage);
  if (c->ha_ws) hipFree(c->ha_ws);
  delete c;
}

int fpc_load_weights(fpc_ctx* c, const fpc_tensor* tensors, int n) {
  if (!c || !tensors || n <= 0) return FPC_E_INVALID;
  TensorMap m;
  for (int i = 0; i < n; ++i) {
    if (!tensors[i].name || tensors[i].ndim < 0 || tensors[i].ndim > 4) return FPC_E_INVALID;
    HostTensor t;
    t.data = tensors[i].data;
    t.shape.assign(tensors[i].shape, tensors[i].shape + tensors[i].ndim);
    m[tensors[i].name] = t;
  }
  std::string missing;
  const int rc = pack_all(c, m, &missing);
  if (rc != FPC_OK) {
    g_hip_err = "checkpoint entry: " + missing;
    return rc;
  }
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipMemcpy(c->blob, c->host_blob.data(), c->blob_floats * sizeof(float), hipMemcpyHostToDevice));
  c->weights_loaded = true;
  return FPC_OK;
}

size_t fpc_packed_size(const fpc_ctx* c) { return c ? c->blob_floats * sizeof(float) : 0; }
void* fpc_packed_device_ptr(fpc_ctx* c) { return c ? c->blob : nullptr; }

int fpc_export_packed(fpc_ctx* c, void* dst, size_t cap) {
  if (!c || !dst) return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  if (cap < c->blob_floats * sizeof(float)) return FPC_E_CAPACITY;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipMemcpy(dst, c->blob, c->blob_floats * sizeof(float), hipMemcpyDeviceToHost));
  return FPC_OK;
}

int fpc_import_packed(fpc_ctx* c, const void* src, size_t n) {
  if (!c || !src) return FPC_E_INVALID;
  if (n != c->blob_floats * sizeof(float)) {
    g_hip_err = "packed weights: " + std::to_string(n) + " bytes, this context's plan packs " + std::to_string(c->blob_floats * sizeof(float));
    return FPC_E_INVALID;
  }
  if (!check_blob_header(c, static_cast<const uint32_t*>(src), &g_hip_err)) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipMemcpy(c->blob, src, n, hipMemcpyHostToDevice));
  c->weights_loaded = true;
  return FPC_OK;
}

int fpc_import_packed_device(fpc_ctx* c, const void* src_dev, size_t n) {
  if (!c || !src_dev) return FPC_E_INVALID;
  if (n != c->blob_floats * sizeof(float)) {
    g_hip_err = "packed weights: " + std::to_string(n) + " bytes, this context's plan packs " + std::to_string(c->blob_floats * sizeof(float));
    return FPC_E_INVALID;
  }
  HIPCHECK(hipSetDevice(c->cfg.device));
  // the 64-byte tag is checked on the host BEFORE the blob is touched; the bytes themselves never leave the device
  uint32_t h[BLOB_HEADER_FLOATS];
  HIPCHECK(hipMemcpy(h, src_dev, sizeof(h), hipMemcpyDeviceToHost));
  if (!check_blob_header(c, h, &g_hip_err)) return FPC_E_INVALID;
  if (src_dev != (const void*)c->blob) {
    c->weights_loaded = false;
    HIPCHECK(hipMemcpy(c->blob, src_dev, n, hipMemcpyDeviceToDevice));
    HIPCHECK(hipDeviceSynchronize());
  }
  c->weights_loaded = true;
  return FPC_OK;
}

int fpc_mark_weights_loaded(fpc_ctx* c) {
  if (!c) return FPC_E_INVALID;
  // the blob was written in place (a collective into fpc_packed_device_ptr): it must carry this context's tag
  uint32_t h[BLOB_HEADER_FLOATS];
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipMemcpy(h, c->blob, sizeof(h), hipMemcpyDeviceToHost));
  if (!check_blob_header(c, h, &g_hip_err)) {
    c->weights_loaded = false;
    return FPC_E_INVALID;
  }
  c->weights_loaded = true;
  return FPC_OK;
}

uint64_t fpc_plan_hash(const fpc_ctx* c) { return c ? plan_hash(c) : 0; }

int fpc_tile_choice(int what, int H, int W, int frames, unsigned plan_flags) {
  const bool r6 = !(plan_flags & FPC_PLAN_TILES_ROUND5);
  if (H <= 0 || W <= 0 || frames <= 0) return FPC_E_INVALID;
  switch (what) {
    case 0: {
      const WKindInfo& k = g_wkinds[w36_kind(128, H, W)];
      return r6 ? w36_stacked_rows(H, W, frames, WK_W36S_C128_4x4, ((H + k.TH - 1) / k.TH) * ((W + k.TW - 1) / k.TW)) : 0;
    }
    case 1: { const WKindInfo& k = g_wkinds[w36_kind(64, H, W, true, r6)]; return 100 * k.TH + k.TW; }
    case 2: {
      const BKind k5 = BK_B320_s2_K32_C128, k6 = BK_B416_s2_K32_C128;
      const BKindInfo& k = g_bkinds[r6 && block_rows(k6, H, W) < block_rows(k5, H, W) ? k6 : k5];
      return 100 * k.TH + k.TW;
    }
  }
  return FPC_E_INVALID;
}

int fpc_check_guards(fpc_ctx* c, long long* bad_words) {
  if (!c || !bad_words) return FPC_E_INVALID;
  *bad_words = 0;
  if (!c->opt.guard_zones || c->slab.zones.empty()) return FPC_E_INVALID;      // the context was not created with FPC_PLAN_GUARD_ZONES
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipDeviceSynchronize());
  unsigned long long* d = nullptr;
  HIPCHECK(hipMalloc((void**)&d, sizeof(*d)));
  {
    const hipError_t e0 = hipMemset(d, 0, sizeof(*d));
    if (e0 != hipSuccess) hipFree(d);
    HIPCHECK(e0);
  }
  for (const Slab* s : c->slabs) count_zones(c->stream, *s, d);      // (a slab that was never reserved has no zones)
  unsigned long long h = 0;
  const hipError_t e1 = hipStreamSynchronize(c->stream);
  const hipError_t e2 = hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost);
  hipFree(d);
  HIPCHECK(e1);
  HIPCHECK(e2);
  *bad_words = (long long)h;
  return FPC_OK;
}

// RCCL is resolved at run time: first among the libraries the process already holds (a torch host has
// torch/lib/librccl.so mapped; the communicator the caller passes came from THAT copy), then the system's.
namespace {
typedef int (*nccl_bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_rank_fn)(void*, int*);
struct RcclApi {
  nccl_bcast_fn bcast = nullptr;
  nccl_rank_fn user_rank = nullptr;
  bool tried = false;
};
static RcclApi g_rccl;
static bool load_rccl() {
  if (g_rccl.tried) return g_rccl.bcast && g_rccl.user_rank;
  g_rccl.tried = true;
  void* h = nullptr;
  void* f = dlsym(RTLD_DEFAULT, "ncclBroadcast");
  if (!f) {
    h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return false;
    f = dlsym(h, "ncclBroadcast");
  }
  g_rccl.bcast = reinterpret_cast<nccl_bcast_fn>(f);
  void* r = h ? dlsym(h, "ncclCommUserRank") : dlsym(RTLD_DEFAULT, "ncclCommUserRank");
  g_rccl.user_rank = reinterpret_cast<nccl_rank_fn>(r);
  return g_rccl.bcast && g_rccl.user_rank;
}
}  // namespace

int fpc_broadcast_weights(fpc_ctx* c, void* nccl_comm, int root) {
  if (!c || !nccl_comm || root < 0) return FPC_E_INVALID;
  if (!load_rccl()) {
    g_hip_err = "librccl.so (ncclBroadcast / ncclCommUserRank) could not be resolved";
    return FPC_E_HIP;
  }
  HIPCHECK(hipSetDevice(c->cfg.device));
  int rank = -1;
  if (g_rccl.user_rank(nccl_comm, &rank) != 0 || rank < 0) {
    g_hip_err = "ncclCommUserRank failed";
    return FPC_E_HIP;
  }
  const bool is_root = rank == root;
  // Step 1: the 64-byte tag alone, into scratch -- every rank learns what the root is about to send BEFORE the
  // collective whose size depends on it.  A root without weights sends a tag with the weights-present flag clear.
  // (the tag's device buffer is 64 bytes of the slab carved at fpc_create: an allocation HERE could fail on one rank,
  // which would return early and leave the others waiting in the collective)
  uint32_t* tag_dev = c->bcast_tag;
  uint32_t tag[BLOB_HEADER_FLOATS];
  if (is_root) {
    fill_blob_header(c, tag);
    if (!c->weights_loaded) tag[8] = 0;
    hipMemcpyAsync(tag_dev, tag, sizeof(tag), hipMemcpyHostToDevice, c->stream);
  }
  int nrc = g_rccl.bcast(tag_dev, tag_dev, sizeof(tag), /*ncclUint8*/ 1, root, nccl_comm, c->stream);
  hipError_t he = hipMemcpyAsync(tag, tag_dev, sizeof(tag), hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (nrc != 0 || he != hipSuccess) {
    g_hip_err = nrc ? "ncclBroadcast(tag) failed: ncclResult " + std::to_string(nrc) : std::string("tag copy: ") + hipGetErrorString(he);
    return FPC_E_HIP;
  }
  if (tag[0] != BLOB_MAGIC || tag[8] != 1) {   // every rank sees the same tag: all return here, no rank is left in step 2
    g_hip_err = "the root rank holds no packed weights (load them on the root before fpc_broadcast_weights)";
    return FPC_E_NO_WEIGHTS;
  }
  // Step 2: the blob, `root_bytes` long on EVERY rank.  A rank whose own plan differs still takes part (into scratch), so
  // that no rank is left waiting in the collective; it then reports the mismatch.
  const size_t root_bytes = (((size_t)tag[7] << 32) | tag[6]) * sizeof(float);
  std::string why;
  const bool match = check_blob_header(c, tag, &why);
  void* dst = c->blob;
  void* scratch = nullptr;
  bool slab_used = false;
  if (!match) {
    // Somewhere to receive root_bytes.  What this rank must NOT do is return before the collective (the others would wait
    // in ncclBroadcast until the backend's time-out), so three places are tried: scratch memory; this rank's own blob
    // when it is large enough (its weights are declared gone BEFORE the bytes arrive -- a broadcast that fails half way
    // leaves the blob undefined); the activation workspace, which holds nothing between calls and is re-zeroed after.
    if (hipMalloc(&scratch, root_bytes) == hipSuccess) {
      dst = scratch;
    } else {
      (void)hipGetLastError();
      scratch = nullptr;
      if (root_bytes <= c->blob_floats * sizeof(float)) {
        c->weights_loaded = false;
      } else if (root_bytes <= c->slab.bytes) {
        dst = c->slab.base;
        slab_used = true;
      } else {
        g_hip_err = "no memory to take part in the weight broadcast (" + std::to_string(root_bytes) + " bytes: no scratch, and neither this "
                    "context's blob nor its workspace is that large); the other ranks of this communicator will wait for this one";
        return FPC_E_HIP;
      }
    }
  }
  nrc = g_rccl.bcast(dst, dst, root_bytes, 1, root, nccl_comm, c->stream);
  he = hipStreamSynchronize(c->stream);
  if (scratch) hipFree(scratch);
  if (slab_used) {      // foreign bytes in the workspace: back to the state fpc_create left (zeros, canary zones)
    hipMemsetAsync(c->slab.base, 0, std::min(c->slab.bytes, align_up(root_bytes, 256)), c->stream);
    hipStreamSynchronize(c->stream);
    if (c->opt.guard_zones) fill_guards(c);
  }
  if (nrc != 0 || he != hipSuccess) {
    if (match) c->weights_loaded = false;      // the blob may hold part of the new bytes
    g_hip_err = nrc ? "ncclBroadcast(weights) failed: ncclResult " + std::to_string(nrc) : std::string("broadcast: ") + hipGetErrorString(he);
    return FPC_E_HIP;
  }
  if (!match) {
    g_hip_err = why;
    return FPC_E_INVALID;
  }
  c->weights_loaded = true;
  return FPC_OK;
}

int fpc_set_stream(fpc_ctx* c, void* s) {
  if (!c) return FPC_E_INVALID;
  // the stream the ctx already runs on -- the caller's from an earlier call, or the ctx's OWN one handed back (fpc_get_stream):
  // nothing to do, and ownership stays as it is (round 5's first form destroyed the ctx's own stream in the second case and
  // went on with the dangling handle)
  if ((hipStream_t)s == c->stream) return FPC_OK;
  HIPCHECK(hipSetDevice(c->cfg.device));
  std::lock_guard<std::mutex> queue_lock(qmap::state().mu);
  if (c->own_stream && c->stream) {
    hipStreamSynchronize(c->stream);
    hipStreamDestroy(c->stream);
  }
  c->stream = (hipStream_t)s;
  c->own_stream = false;
  // The registry's entry is THIS context's main slot -- never another context's that happens to name the same caller
  // stream.  The caller's stream is a foreign object: its queue class is looked up in a small per-context memo of handles
  // seen before, and otherwise found with ONE probe round (a one-thread kernel of ~40 us on it) only if that is safe --
  // probing on, not the null stream, not being captured into a graph, and idle.  Anything else: class unknown, the
  // context's other streams stay as they are.
  qmap::Placed* mainp = qmap::find(c, SLOT_MAIN);
  int k = qmap::Q_UNKNOWN;
  qmap::DeviceQueues& q = qmap::state().dev[c->cfg.device];
  bool memo_hit = false;
  for (const auto& m : c->caller_stream_memo)
    if (m.first == c->stream) { k = m.second; memo_hit = true; }
  if (!memo_hit && c->queue_probe && c->stream && !q.futile && q.anchor.size() >= 2) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(c->stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    if (!capturing && hipStreamQuery(c->stream) == hipSuccess) {
      k = qmap::classify(q, c->stream);
      if (k == qmap::Q_INCONCLUSIVE) k = qmap::Q_UNKNOWN;
      if (c->caller_stream_memo.size() >= 4) c->caller_stream_memo.erase(c->caller_stream_memo.begin());
      c->caller_stream_memo.push_back({c->stream, k});
    }
    (void)hipGetLastError();
  }
  if (mainp) {
    mainp->st = c->stream;
    mainp->qclass = k;
  }
  // a sub-batch or side stream of this context on the caller's queue would run in a row with it: exchanged
  if (k >= 0) {
    auto settle = [&](hipStream_t& st, int slot, bool heavy) {
      qmap::Placed* p = qmap::find(c, slot);
      if (!st || !p || p->qclass != k) return;
      const qmap::Placed old = *p;
      for (size_t i = 0; i < qmap::state().placed.size(); ++i)      // (out of the table while its replacement is chosen)
        if (&qmap::state().placed[i] == p) { qmap::state().placed.erase(qmap::state().placed.begin() + i); break; }
      hipStream_t fresh = qmap::acquire(c->cfg.device, c, slot, heavy, true, true);
      if (fresh) {
        hipStreamSynchronize(st);
        hipStreamDestroy(st);
        st = fresh;
      } else {
        qmap::state().placed.push_back(old);
      }
    };
    for (size_t i = 0; i < c->aux.size(); ++i) settle(c->aux[i], SLOT_AUX + (int)i, true);
    for (size_t i = 0; i < c->side.size(); ++i) settle(c->side[i], SLOT_SIDE + (int)i, false);
  }
  return FPC_OK;
}

void* fpc_get_stream(fpc_ctx* c) { return c ? (void*)c->stream : nullptr; }

void* fpc_upload_stream(fpc_ctx* c) {
  if (!c) return nullptr;
  if (c->upload) return (void*)c->upload;
  if (hipSetDevice(c->cfg.device) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> queue_lock(qmap::state().mu);
  // beside this context's main / sub-batch streams (its side streams carry the few-CU NMS launches: sharing a queue with
  // one of them is the lesser evil when all four queues are taken) and, where a queue is left, other contexts' too
  c->upload = qmap::acquire(c->cfg.device, c, SLOT_UPLOAD, false, c->queue_probe, false);
  return (void*)c->upload;
}

int fpc_stream_report(fpc_ctx* c, fpc_stream_report_t* out) {
  if (!c || !out) return FPC_E_INVALID;
  memset(out, 0, sizeof(*out));
  std::lock_guard<std::mutex> queue_lock(qmap::state().mu);
  const qmap::DeviceQueues& q = qmap::state().dev[c->cfg.device];
  out->probing = c->queue_probe && !q.futile ? 1 : 0;
  out->hw_queues_found = (int)q.anchor.size();
  out->process_probe_rounds = q.rounds;
  out->process_probe_launches = q.launches;
  out->process_probe_ms = (float)q.ms;
  out->process_inconclusive_rounds = q.inconclusive;
  out->create_probe_rounds = c->probe_rounds;
  out->create_placement_ms = (float)c->placement_ms;
  out->process_registered_streams = (int)qmap::state().placed.size();
  for (const qmap::Placed& p : qmap::state().placed) {
    if (p.owner != c || out->n_streams >= 16) continue;
    out->slot[out->n_streams] = p.slot;
    out->queue[out->n_streams] = p.qclass;
    out->n_streams += 1;
  }
  return FPC_OK;
}

int fpc_sync(fpc_ctx* c) {
  if (!c) return FPC_E_INVALID;
  HIPCHECK(hipStreamSynchronize(c->stream));
#ifdef FPC_DIAG
  if (c->diag_stamps && c->diag_n) {
    if (FILE* f = fopen(getenv("FPC_STAMP_FILE") ? getenv("FPC_STAMP_FILE") : "/tmp/fpc_stamps.bin", "wb")) {
      fwrite(c->diag_stamps, sizeof(unsigned long long) * 8, getenv("FPC_STAMP_FULL") ? 65536 : c->diag_n, f);
      fclose(f);
    }
  }
#endif
  return FPC_OK;
}

int fpc_forward(fpc_ctx* c, const float* frames, int n, float* prob, float* desc, float* logits) {
  if (!c) return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  if (n < 1 || n > c->B || !frames) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const bool de = c->cfg.descriptor_enabled != 0;
  if (c->split_f16) HIPCHECK(hipMemsetAsync(c->status + 1, 0, sizeof(int32_t), c->stream));
  int rc = for_each_sub(c, n, [&](const Sub& sb) { run_path(c, frames, sb, de, 0); });
  if (rc != FPC_OK) return rc;
  const int HWc = c->Hc * c->Wc;
  if (prob) HIPCHECK(hipMemcpyAsync(prob, c->prob, (size_t)n * c->H * c->W * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  if (logits) {
    const size_t tot = (size_t)n * 65 * HWc;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, c->lg, c->lgcs, 65,
                       HWc, n, logits, (uint32_t*)nullptr, 0);
  }
  if (desc) {
    const size_t tot = (size_t)n * c->D * HWc;
    if (de && c->bf16)
      hipLaunchKernelGGL(nhwc_bf16_to_nchw_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                         reinterpret_cast<const unsigned short*>(c->desc_map), c->D, c->D, HWc, n, desc);
    else if (de)
      hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                         c->desc_map, c->D, c->D, HWc, n, desc, c->range, (int)RANGE_MAX_DESC);
    else  // superpoint.py:106-109: zeros when the descriptor head is disabled
      HIPCHECK(hipMemsetAsync(desc, 0, tot * sizeof(float), c->stream));
  }
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

// ... of the C++ network: the tensors build_vgg_plan listed (no "desc_a" / "desc_b" with the descriptor head disabled)
static int read_vgg_activation(fpc_ctx* c, const char* name, int frame0, int n, float* out, int* channels, int* height, int* width) {
  for (const fpc_ctx::VTap& t : c->vtaps) {
    if (strcmp(t.name, name)) continue;
    if (!strcmp(name, "det_b") && !c->logits_valid) return FPC_E_INVALID;
    if (channels) *channels = t.C;
    if (height) *height = t.H;
    if (width) *width = t.W;
    if (!out || n == 0) return FPC_OK;
    HIPCHECK(hipSetDevice(c->cfg.device));
    const int HW = t.H * t.W;
    const size_t tot = (size_t)n * t.C * HW;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       t.p + (size_t)frame0 * HW * t.cs, t.cs, t.C, HW, n, out, (uint32_t*)nullptr, 0);
    HIPCHECK(hipGetLastError());
    return FPC_OK;
  }
  return FPC_E_INVALID;
}

// Tensors the last forward left in the workspace, by the reference module that produced them.
int fpc_read_activation(fpc_ctx* c, const char* name, int frame0, int n, float* out, int* channels, int* height, int* width) {
  if (!c || !name || frame0 < 0 || n < 0 || frame0 + n > c->B) return FPC_E_INVALID;
  if (c->vgg) return read_vgg_activation(c, name, frame0, n, out, channels, height, width);
  const int H4 = c->H / 4, W4 = c->W / 4, Hc = c->Hc, Wc = c->Wc, H16 = c->H / 16, W16 = c->W / 16;
  const bool lowp = c->bf16;          // bf16 tensors (all but the logits)
  struct Tap { const char* name; const void* p; int cs, C, H, W; bool bf; int off; };
  const Tap taps[] = {
      {"pool", c->x0, 64, 64, H4, W4, lowp, 0},
      {"layer1.0", c->x1, 64, 64, H4, W4, lowp, 0},
      {"layer1.1", c->x2, 64, 64, H4, W4, lowp, 0},
      {"layer2.0", c->x3, 128, 128, Hc, Wc, lowp, 0},
      {"layer2.1", c->cat, 256, 128, Hc, Wc, lowp, 128},
      {"det.0", c->d0, (c->bf16 || c->split) ? 80 : 72, 65, Hc, Wc, lowp, 0},
      {"det.1", c->lg, c->lgcs, 65, Hc, Wc, false, 0},
      {"desc_in.0", c->y16a, 256, 256, H16, W16, lowp, 0},
      {"desc_in.1", c->y16b, 256, 256, H16, W16, lowp, 0},
      {"up", c->cat, 256, 128, Hc, Wc, lowp, 0},
      {"desc_out.0", c->lo0, 128, 128, Hc, Wc, lowp, 0},
      {"desc_out.1", c->desc_map, 128, 128, Hc, Wc, lowp, 0},
  };
  for (const Tap& t : taps) {
    if (strcmp(t.name, name)) continue;
    if (!c->cfg.descriptor_enabled && (!strncmp(name, "desc", 4) || !strcmp(name, "up"))) return FPC_E_INVALID;
    // FPC_BF16's fpc_detect fuses exp-softmax into detector.layer.1: that call writes NMS state and candidates, no logits
    if (!strcmp(name, "det.1") && !c->logits_valid) return FPC_E_INVALID;
    if (channels) *channels = t.C;
    if (height) *height = t.H;
    if (width) *width = t.W;
    if (!out || n == 0) return FPC_OK;
    HIPCHECK(hipSetDevice(c->cfg.device));
    const int HW = t.H * t.W;
    const size_t tot = (size_t)n * t.C * HW;
    const dim3 grid((unsigned)((tot + 255) / 256));
    if (t.bf) {
      const unsigned short* src = static_cast<const unsigned short*>(t.p) + t.off + (size_t)frame0 * HW * t.cs;
      hipLaunchKernelGGL(nhwc_bf16_to_nchw_kernel, grid, dim3(256), 0, c->stream, src, t.cs, t.C, HW, n, out);
    } else {
      const float* src = static_cast<const float*>(t.p) + t.off + (size_t)frame0 * HW * t.cs;
      hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, c->stream, src, t.cs, t.C, HW, n, out, (uint32_t*)nullptr, 0);
    }
    HIPCHECK(hipGetLastError());
    return FPC_OK;
  }
  return FPC_E_INVALID;
}

int fpc_detect(fpc_ctx* c, const float* frames, int n) {
  if (!c) return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  if (n < 1 || n > c->B || !frames) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const bool de = c->cfg.descriptor_enabled != 0;
  if (c->split_f16) HIPCHECK(hipMemsetAsync(c->status + 1, 0, sizeof(int32_t), c->stream));
  c->pts_n = 0;
  const int rc = for_each_sub(c, n, [&](const Sub& sb) { run_path(c, frames, sb, de, 1); });
  if (rc == FPC_OK) {
    c->pts_n = n;
    c->pts_desc = de;
  }
  return rc;
}

int fpc_detect_u8(fpc_ctx* c, const uint8_t* frames, int n, int layout) {
  if (!c || !frames || n < 1 || n > c->B || layout < FPC_U8_GRAY || layout > FPC_U8_BGR_HWC_GRAY) return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  const int cout = (layout == FPC_U8_GRAY || layout == FPC_U8_BGR_HWC_GRAY) ? 1 : 3;
  if (cout != c->cin) return FPC_E_INVALID;  // gray layouts feed an in_channels = 1 ctx, colour layouts a 3-channel one
  HIPCHECK(hipSetDevice(c->cfg.device));
  const int HW = c->H * c->W;  // multiple of 64 (H, W multiples of 8)
  if (!c->u8stage) HIPCHECK(hipMalloc((void**)&c->u8stage, (size_t)c->B * c->cin * HW * sizeof(float)));
  const size_t quads = (size_t)n * (HW / 4);
  hipLaunchKernelGGL(u8_to_float_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, c->stream, frames,
                     c->u8stage, n, HW, layout);
  return fpc_detect(c, c->u8stage, n);
}

const float* fpc_u8_staging(fpc_ctx* c) { return c ? c->u8stage : nullptr; }

int fpc_detect_u8_resized(fpc_ctx* c, const uint8_t* frames, int n, int src_h, int src_w, int layout) {
  if (!c || !frames || n < 1 || n > c->B || src_h < 2 || src_w < 2 || src_h > 16384 || src_w > 16384 ||
      (layout != FPC_U8_RGB_HWC && layout != FPC_U8_BGR_HWC) || c->cin != 3)
    return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t HW = (size_t)c->H * c->W;
  if (!c->u8stage) HIPCHECK(hipMalloc((void**)&c->u8stage, (size_t)c->B * c->cin * HW * sizeof(float)));
  ResizeArgs a{};
  a.in = frames;
  a.out = c->u8stage;
  a.n = n; a.src_h = src_h; a.src_w = src_w; a.H = c->H; a.W = c->W;
  // make_query_image, python/src/inference.py:72-85 (Python float = double; int() truncates)
  const double scale_h = (double)c->H / src_h, scale_w = (double)c->W / src_w;
  const double scale_max = scale_h > scale_w ? scale_h : scale_w;
  a.new_w = (int)(src_w * scale_max);
  a.new_h = (int)(src_h * scale_max);
  if (a.new_w < c->W || a.new_h < c->H) return FPC_E_INVALID;  // the reference's crop would come out short
  a.x0 = a.new_w / 2 - c->W / 2;
  a.y0 = a.new_h / 2 - c->H / 2;
  a.scale_x = 1.0 / ((double)a.new_w / src_w);   // cv::resize: inv_scale = dsize / ssize, scale = 1 / inv_scale
  a.scale_y = 1.0 / ((double)a.new_h / src_h);
  a.swap_rb = layout == FPC_U8_BGR_HWC;
  const size_t tot = (size_t)n * HW;
  hipLaunchKernelGGL(resize_crop_u8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, a);
  return fpc_detect(c, c->u8stage, n);
}

// 3x3 inverse of a flat homography (h[8], implicit 1), normalised back to flat form -- invert_homography,
// python/src/homographies.py:185-209 (torch.linalg.inv in fp32 there, double here)
static bool invert_flat_homography(const float* h, float* out) {
  const double m[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[2] * m[7] - m[1] * m[8], c02 = m[1] * m[5] - m[2] * m[4];
  const double c10 = m[5] * m[6] - m[3] * m[8], c11 = m[0] * m[8] - m[2] * m[6], c12 = m[2] * m[3] - m[0] * m[5];
  const double c20 = m[3] * m[7] - m[4] * m[6], c21 = m[1] * m[6] - m[0] * m[7], c22 = m[0] * m[4] - m[1] * m[3];
  const double det = m[0] * c00 + m[1] * c10 + m[2] * c20;
  if (!(std::fabs(det) > 1e-300) || !(std::fabs(c22) > 0.0)) return false;
  const double inv[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};  // adjugate; the 1/det cancels in mat2flat
  for (int i = 0; i < 8; ++i) out[i] = (float)(inv[i] / inv[8]);
  return true;
}

int fpc_homography_adaptation(fpc_ctx* c, const float* frames, int n, const float* homographies, const float* inverses,
                              int num, int erosion_radius, int aggregation, float* prob_out) {
  if (!c || !frames || !prob_out || n < 1 || n > c->B || num < 0 || (num > 0 && !homographies) || erosion_radius < 0 ||
      erosion_radius > 64 || (aggregation != 0 && aggregation != 1))
    return FPC_E_INVALID;
  if (!c->weights_loaded) return FPC_E_NO_WEIGHTS;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const bool de = c->cfg.descriptor_enabled != 0;
  const size_t HW = (size_t)c->H * c->W, frame_elems = (size_t)c->cin * HW;
  // workspace: warped frames [B,cin,HW] | warped prob [B,HW] | sum [B,HW] | max [B,HW] | cnt, count, mask, tmp [HW] each
  if (!c->ha_ws)
    HIPCHECK(hipMalloc((void**)&c->ha_ws, ((size_t)c->B * frame_elems + 3 * (size_t)c->B * HW + 4 * HW) * sizeof(float)));
  float* wfr = reinterpret_cast<float*>(c->ha_ws);
  float* wprob = wfr + (size_t)c->B * frame_elems;
  float* sum = wprob + (size_t)c->B * HW;
  float* mx = sum + (size_t)c->B * HW;
  float* cnt = mx + (size_t)c->B * HW;
  float* count = cnt + HW;
  float* mask = count + HW;
  float* tmp = mask + HW;
  const dim3 gp((unsigned)((HW + 255) / 256)), bp(256);
  hipStream_t st = c->stream;
  auto forward = [&](const float* f) -> int {  // prob maps of n frames -> c->prob (the path up to depth-to-space)
    return for_each_sub(c, n, [&](const Sub& sb) { run_path(c, f, sb, de, 0); });
  };
  int rc = forward(frames);  // all_probs = net(image), all_counts = 1   (homographies.py:269-270)
  if (rc != FPC_OK) return rc;
  WarpCoeffs none{};
  hipLaunchKernelGGL(unwarp_accumulate_kernel, gp, bp, 0, st, c->prob, none, count, sum, mx, cnt, n, c->H, c->W, 1);
  for (int i = 0; i < num; ++i) {
    WarpCoeffs k{}, kinv{};
    memcpy(k.c, homographies + (size_t)i * 8, sizeof(k.c));
    if (inverses) memcpy(kinv.c, inverses + (size_t)i * 8, sizeof(kinv.c));
    else if (!invert_flat_homography(k.c, kinv.c)) return FPC_E_INVALID;
    // warped = transform(image, H); count = transform(ones, H_inv, nearest); mask = transform(ones, H, nearest)  :288-292
    hipLaunchKernelGGL(warp_perspective_kernel, gp, bp, 0, st, frames, wfr, n * c->cin, c->H, c->W, k, 0, 0);
    float* cdst = erosion_radius ? tmp : count;
    hipLaunchKernelGGL(warp_perspective_kernel, gp, bp, 0, st, (const float*)nullptr, cdst, 1, c->H, c->W, kinv, 1, 1);
    if (erosion_radius) hipLaunchKernelGGL(erode_ellipse_kernel, gp, bp, 0, st, tmp, count, c->H, c->W, erosion_radius);
    float* mdst = erosion_radius ? tmp : mask;
    hipLaunchKernelGGL(warp_perspective_kernel, gp, bp, 0, st, (const float*)nullptr, mdst, 1, c->H, c->W, k, 1, 1);
    if (erosion_radius) hipLaunchKernelGGL(erode_ellipse_kernel, gp, bp, 0, st, tmp, mask, c->H, c->W, erosion_radius);
    rc = forward(wfr);  // warped_prob = net(warped)   :297
    if (rc != FPC_OK) return rc;
    HIPCHECK(hipMemcpyAsync(wprob, c->prob, (size_t)n * HW * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(mul_mask_kernel, gp, bp, 0, st, wprob, mask, n, HW);                         // :298
    hipLaunchKernelGGL(unwarp_accumulate_kernel, gp, bp, 0, st, wprob, kinv, count, sum, mx, cnt, n, c->H, c->W, 0);  // :299-305
  }
  hipLaunchKernelGGL(aggregate_kernel, gp, bp, 0, st, sum, mx, cnt, prob_out, n, HW, (float)(num / 3), aggregation);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_get_points(fpc_ctx* c, const float* prob, const float* desc_nchw, int n) {
  if (!c || !prob || n < 1 || n > c->B) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const int HW = c->H * c->W;
  HIPCHECK(hipMemsetAsync(c->ncand, 0, sizeof(int32_t) * c->B, c->stream));
  // (the per-frame range words belong to the last CALL: a caller-provided map has no input frames to flag, and an earlier
  // fpc_detect's FPC_E_NONFINITE must not come back from this call's fpc_get_counts)
  HIPCHECK(hipMemsetAsync(c->range, 0, sizeof(uint32_t) * FPC_RANGE_WORDS * c->B, c->stream));
  HIPCHECK(hipMemsetAsync(c->rowmax, 0, sizeof(float) * c->Hc * c->B, c->stream));
  const int per = (HW + 255) / 256;
  hipLaunchKernelGGL(threshold_kernel, dim3(per * n), dim3(256), 0, c->stream, prob, n, HW, c->cfg.conf_thresh,
                     c->nmsmap, c->cand, c->ncand);
  Sub all;
  all.f0 = 0;
  all.n = n;
  all.st = c->stream;
  run_nms(c, all);
  if (desc_nchw && c->cfg.descriptor_enabled) {
    const size_t tot = (size_t)n * c->D * c->Hc * c->Wc;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, desc_nchw,
                       c->D, c->Hc * c->Wc, n, c->desc_in_nhwc);
    run_desc(c, all, c->desc_in_nhwc);
  }
  HIPCHECK(hipGetLastError());
  c->pts_n = n;
  c->pts_desc = desc_nchw && c->cfg.descriptor_enabled;
  return FPC_OK;
}

int fpc_sample_descriptors(fpc_ctx* c, const float* desc_nchw, const double* xy, int k, float* out) {
  if (!c || !desc_nchw || k < 0 || (k > 0 && (!xy || !out))) return FPC_E_INVALID;
  if (k == 0) return FPC_OK;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t tot = (size_t)c->D * c->Hc * c->Wc;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, desc_nchw, c->D,
                     c->Hc * c->Wc, 1, c->desc_in_nhwc);
  if (c->D == 256)
    hipLaunchKernelGGL(descriptor_at_points_kernel<4>, dim3((k + 3) / 4), dim3(256), 0, c->stream, c->desc_in_nhwc, 256,
                       c->Hc, c->Wc, c->H, c->W, xy, k, out);
  else
    hipLaunchKernelGGL(descriptor_at_points_kernel<2>, dim3((k + 3) / 4), dim3(256), 0, c->stream, c->desc_in_nhwc, 128,
                       c->Hc, c->Wc, c->H, c->W, xy, k, out);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_match(fpc_ctx* c, const float* q, int nq, const float* t, int nt, int cross_check, float max_dist,
              int32_t* match, float* dist) {
  if (!c || nq < 0 || nt < 0 || nq > c->cap || nt > c->cap || (!q && nq) || (!t && nt) || (!match && nq))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  if (nq == 0) return FPC_OK;
  HIPCHECK(hipMemsetAsync(c->rowbest, 0xff, sizeof(unsigned long long) * nq, c->stream));
  if (nt == 0) {  // no train rows: the finalize kernel on an untouched rowbest writes -1 / +inf (it reads no colbest then)
    hipLaunchKernelGGL(match_finalize_kernel, dim3((nq + 255) / 256), dim3(256), 0, c->stream, c->rowbest, c->colbest, nq,
                       cross_check, max_dist, match, dist);
    HIPCHECK(hipGetLastError());
    return FPC_OK;
  }
  HIPCHECK(hipMemsetAsync(c->colbest, 0xff, sizeof(unsigned long long) * nt, c->stream));
  MatchArgs a{};
  a.q = q; a.t = t; a.nq = nq; a.nt = nt; a.D = c->D; a.rowbest = c->rowbest; a.colbest = c->colbest; a.first = nullptr; a.tol2 = -1.f;
  hipLaunchKernelGGL(match_gemm_kernel, dim3((nq + 127) / 128, (nt + 127) / 128), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(match_finalize_kernel, dim3((nq + 255) / 256), dim3(256), 0, c->stream, c->rowbest, c->colbest, nq,
                     cross_check, max_dist, match, dist);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_first_within(fpc_ctx* c, const float* key, int nk, const float* cur, int nc, float tolerance, int32_t* first) {
  if (!c || nk < 0 || nc < 0 || nk > c->cap || nc > c->cap || !(tolerance >= 0.f) || (!key && nk) || (!cur && nc) ||
      (!first && nk))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  if (nk == 0) return FPC_OK;
  if (nc == 0) {
    HIPCHECK(hipMemsetAsync(first, 0xff, sizeof(int32_t) * nk, c->stream));
    return FPC_OK;
  }
  unsigned int* ws = reinterpret_cast<unsigned int*>(c->rowbest);
  HIPCHECK(hipMemsetAsync(ws, 0xff, sizeof(unsigned int) * nk, c->stream));
  MatchArgs a{};
  a.q = key; a.t = cur; a.nq = nk; a.nt = nc; a.D = c->D; a.rowbest = nullptr; a.colbest = nullptr; a.first = ws; a.tol2 = tolerance * tolerance;
  hipLaunchKernelGGL(match_gemm_kernel, dim3((nk + 127) / 128, (nc + 127) / 128), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(first_finalize_kernel, dim3((nk + 255) / 256), dim3(256), 0, c->stream, ws, nk, first);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

// Argument checks of the entry points below (include/fpc.h).  A NaN max_dist or ratio fails its comparison: refused.
static bool pairing_ok(int pairing) { return pairing == FPC_PAIR_KEY || pairing == FPC_PAIR_PREVIOUS; }
static bool frames_ok(const fpc_ctx* c, int n) { return n >= 1 && n <= c->pts_n && n <= c->B; }
static bool gate_ok(float max_dist, float ratio) { return max_dist >= 0.f && ratio >= 0.f && ratio <= 1.f; }

// ... and of those that read the frames' descriptors, with or without a key set
static int match_frames_check(fpc_ctx* c, int n, const float* key, const int32_t* nkey) {
  if (!c->cfg.descriptor_enabled || !c->pts_desc || !frames_ok(c, n)) return FPC_E_INVALID;
  if (key && (!nkey || (reinterpret_cast<uintptr_t>(key) & 15))) return FPC_E_INVALID;   // rows are read as float4
  return FPC_OK;
}

static MatchFramesArgs match_frames_args(fpc_ctx* c, int n, const float* key, const int32_t* nkey) {
  MatchFramesArgs a{};
  a.desc = c->desc_out; a.count = c->count; a.key = key; a.nkey = key ? nkey : nullptr;
  a.n = n; a.cap = c->cap; a.D = c->D;
  a.norms = c->mf_norms; a.top2 = c->mf_top2; a.colbest = c->mf_colbest;
  return a;
}

int fpc_match_frames(fpc_ctx* c, int n, int pairing, const float* key, const int32_t* nkey, int cross_check,
                     float max_dist, float ratio, int32_t* match, float* dist) {
  if (!c || !match || !pairing_ok(pairing) || !gate_ok(max_dist, ratio) || (pairing == FPC_PAIR_KEY && !key))
    return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, key, nkey)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, key, nkey);
  a.pairing = pairing;
  a.cross_check = cross_check != 0;
  if (a.cross_check)
    HIPCHECK(hipMemsetAsync(c->mf_colbest, 0xff, sizeof(unsigned long long) * n * c->cap, c->stream));
  hipLaunchKernelGGL(mf_norms_kernel, dim3((c->cap + 127) / 128, n + 1), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(match_frames_kernel, dim3((c->cap + MF_ROWS - 1) / MF_ROWS, n), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(match_frames_finalize_kernel, dim3((c->cap + 255) / 256, n), dim3(256), 0, c->stream, a, max_dist,
                     ratio, match, dist);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_first_within_frames(fpc_ctx* c, int n, const float* key, const int32_t* nkey, float tolerance, int32_t* first) {
  if (!c || !first || !key || !nkey || !(tolerance >= 0.f)) return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, key, nkey)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, key, nkey);
  a.first_mode = 1;
  a.tol2 = tolerance * tolerance;
  a.first = first;
  hipLaunchKernelGGL(mf_norms_kernel, dim3((c->cap + 127) / 128, n + 1), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(match_frames_kernel, dim3((c->cap + MF_ROWS - 1) / MF_ROWS, n), dim3(256), 0, c->stream, a);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_default_ransac_params(fpc_ransac_params* p) {
  if (!p) return FPC_E_INVALID;
  p->iterations = 1024;
  p->reproj_threshold = 3.0f;
  p->seed = 0;
  p->refits = 2;
  p->min_inliers = 8;
  return FPC_OK;
}

// ---- the geometry chain's host path (include/fpc.h): every call below is a pair list -- explicit pairs, the frames' match
// ---- table, or a match table against bank slots -- and its family's solver step behind it ------------------------------------
// field checks of the parameter structs (a NaN fails its comparison: refused); sample: the floor of min_inliers
static bool threshold_ok(float thr) { return thr > 0.f && thr < 1e18f; }
static bool camera_ok(float fx, float fy, float cx, float cy) {
  return std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx > 0.f && fy > 0.f;
}
static bool ransac_fields_ok(int iterations, float thr, int refits, int min_inliers, int sample) {
  return iterations >= 1 && iterations <= HF_MAX_ITERATIONS && threshold_ok(thr) && refits >= 0 && refits <= 4 &&
         min_inliers >= sample;
}
static bool ransac_params_ok(const fpc_ransac_params* p, int sample = 4) {
  return p && ransac_fields_ok(p->iterations, p->reproj_threshold, p->refits, p->min_inliers, sample);
}

// what the pair sources refuse (the PnP calls, whose records and kernels are their own, use these too), and every call's tail
static bool explicit_ok(const fpc_ctx* c, int n, int stride) { return !(n < 1 || n > c->B || stride < 1 || stride > c->cap); }
static bool bank_ok(const fpc_ctx* c, int n, const int32_t* slot, const int32_t* match) {
  return c->bank_slab && slot && match && frames_ok(c, n);
}
static int launched() { HIPCHECK(hipGetLastError()); return FPC_OK; }

// An HfArgs on the pair-list workspace: the context's, one problem per frame; with per_frame = k the top-K reservation's,
// whose n problems are k per frame.  ransac_args adds the RANSAC parameters; the pose calls need none.
static HfArgs hf_args(const fpc_ctx* c, int n, float thr, int per_frame = 0) {
  HfArgs a{};
  a.pairs = per_frame ? c->topk_pairs : c->hf_pairs; a.row = per_frame ? c->topk_row : c->hf_row;
  a.np = per_frame ? c->topk_np : c->hf_np; a.best = per_frame ? c->topk_best : c->hf_best;
  a.cap = c->cap; a.n = n; a.thr = thr; a.per_frame = per_frame;
  return a;
}
static HfArgs ransac_args(const fpc_ctx* c, int n, const fpc_ransac_params* p, int per_frame = 0) {
  HfArgs a = hf_args(c, n, p->reproj_threshold, per_frame);
  a.T = p->iterations; a.refits = p->refits; a.min_inliers = p->min_inliers; a.seed = p->seed;
  return a;
}

// The pair list of a's a.n problems, one helper per source: it checks the source's arguments, selects the device and
// launches the kernel that fills a's workspace.  mask (the caller's inlier rows, zeroed here) may be NULL: the pose calls.
static int pairs_explicit(fpc_ctx* c, const HfArgs& a, const float* src_xy, const float* dst_xy, const int32_t* npairs,
                          int stride, uint8_t* mask) {
  if (!src_xy || !dst_xy || !npairs || !explicit_ok(c, a.n, stride)) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(hf_pack_kernel, dim3((stride + 255) / 256, a.n), dim3(256), 0, c->stream, a, src_xy, dst_xy, npairs,
                     stride, mask);
  return FPC_OK;
}
static int pairs_gather(fpc_ctx* c, const HfArgs& a, int pairing, const int32_t* key_xy, const int32_t* nkey,
                        const int32_t* match, uint8_t* mask, const HfBank& bank = {}) {
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(hf_gather_kernel, dim3(a.n), dim3(256), 0, c->stream, a, c->xy, c->count, pairing, key_xy, nkey, match,
                     mask, bank);
  return FPC_OK;
}
static int pairs_frames(fpc_ctx* c, const HfArgs& a, int pairing, const int32_t* key_xy, const int32_t* nkey,
                        const int32_t* match, uint8_t* mask) {
  if (!match || !pairing_ok(pairing) || !frames_ok(c, a.n) || (pairing == FPC_PAIR_KEY && !key_xy) || (key_xy && !nkey))
    return FPC_E_INVALID;
  return pairs_gather(c, a, pairing, key_xy, nkey, match, mask);     // (no bank: its HfBank is all null)
}
// (n frames; slot and match hold a.n entries: one per frame, or per_frame of them -- fpc_homography_bank_topk)
static int pairs_bank(fpc_ctx* c, const HfArgs& a, int n, const int32_t* slot, const int32_t* match, uint8_t* mask) {
  if (!bank_ok(c, n, slot, match)) return FPC_E_INVALID;
  return pairs_gather(c, a, (int)FPC_PAIR_KEY, c->bank.xy, nullptr, match, mask,
                      HfBank{slot, c->bank.count, c->bank.rows, c->bank.slots});
}

// ---- RANSAC homographies and fundamental matrices (kernels in ransac_homography.h and ransac_fundamental.h): one pack /
// ---- gather kernel, pair record and workspace for both; the 8-point sample needs 8 inliers at the least ------------------------
static int ransac_launch(fpc_ctx* c, const HfArgs& a, float* H, int32_t* ninliers, uint8_t* inlier, int mstride) {
  hipLaunchKernelGGL(ransac_score_kernel, dim3((a.T + 255) / 256, a.n), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(ransac_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, H, ninliers, inlier, mstride);
  return launched();
}
static int fundamental_launch(fpc_ctx* c, const HfArgs& a, float* F, int32_t* ninliers, uint8_t* inlier, int mstride) {
  hipLaunchKernelGGL(fm_score_kernel, dim3((a.T + FM_THREADS - 1) / FM_THREADS, a.n), dim3(FM_THREADS), 0, c->stream, a);
  hipLaunchKernelGGL(fm_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, F, ninliers, inlier, mstride);
  return launched();
}

int fpc_ransac_homography(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                          const fpc_ransac_params* p, float* H, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !H || !ninliers || !ransac_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, inlier)) return rc;
  return ransac_launch(c, a, H, ninliers, inlier, stride);
}

int fpc_homography_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                          const fpc_ransac_params* p, float* H, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !H || !ninliers || !ransac_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, inlier)) return rc;
  return ransac_launch(c, a, H, ninliers, inlier, c->cap);
}

int fpc_ransac_fundamental(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                           const fpc_ransac_params* p, float* F, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !F || !ninliers || !ransac_params_ok(p, FM_SAMPLE)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, inlier)) return rc;
  return fundamental_launch(c, a, F, ninliers, inlier, stride);
}

int fpc_fundamental_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                           const fpc_ransac_params* p, float* F, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !F || !ninliers || !ransac_params_ok(p, FM_SAMPLE)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, inlier)) return rc;
  return fundamental_launch(c, a, F, ninliers, inlier, c->cap);
}

// ---- key-frame bank (include/fpc.h; kernels in match_bank.h) -------------------------------------------------------------
// fpc_match_bank's score pass keeps top-2 keys (16 B) per query row and a column minimum (8 B) per bank row for every
// (frame, slot) pair in flight; the slots run in chunks so that this stays within BANK_WS_BUDGET (one slot at the least).
constexpr size_t BANK_WS_BUDGET = (size_t)256 << 20;

// A FPC_BANK_BF16 bank stores its rows at 2 B per component and adds the call's rounded query sets ([max_batch][cap][D]
// bf16) to the workspace; the chunk formula is the same.
int fpc_bank_create_ex(fpc_ctx* c, int slots, int rows, int format) {
  if (!c || c->bank_slab || !c->cfg.descriptor_enabled || slots < 1 || slots > FPC_BANK_MAX_SLOTS || rows < 1 ||
      rows > c->cap || (format != FPC_BANK_F32 && format != FPC_BANK_BF16))
    return FPC_E_INVALID;
  const bool half = format == FPC_BANK_BF16;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t B = c->B, cap = c->cap, D = c->D;
  const size_t per_slot = B * (cap * 16 + (size_t)rows * 8);
  const int chunk = (int)std::min<size_t>(slots, std::max<size_t>(1, BANK_WS_BUDGET / per_slot));
  // (without a bank, c->bank and c->bank16 hold nulls: the format that is not carved keeps them)
  BankArgs& b = c->bank;
  Carver cv(c);
  if (half) cv.into(&c->bank16.desc, (size_t)slots * rows * D);
  else cv.into(&b.desc, (size_t)slots * rows * D);
  cv.into(&b.xy, (size_t)slots * rows * 2);
  cv.into(&b.count, slots); cv.into(&b.norms, (size_t)slots * rows);
  cv.into(&b.top2, B * chunk * cap * 2); cv.into(&b.colbest, B * chunk * rows);
  cv.into(&b.score, B * slots); cv.into(&b.best, B);
  if (half) cv.into(&c->bank16.q, B * cap * D);
  if (int rc = c->bank_slab.allocate(c->stream, cv)) return rc;           // (zeroed: every slot starts empty)
  c->bank_format = format;
  b.slots = slots; b.rows = rows; b.D = c->D; b.chunk = chunk;
  return FPC_OK;
}

int fpc_bank_create(fpc_ctx* c, int slots, int rows) { return fpc_bank_create_ex(c, slots, rows, FPC_BANK_F32); }

int fpc_bank_format(fpc_ctx* c, int* format, const void** desc) {
  if (!c || !c->bank_slab || (!format && !desc)) return FPC_E_INVALID;
  if (format) *format = c->bank_format;
  if (desc) *desc = c->bank_format == FPC_BANK_BF16 ? (const void*)c->bank16.desc : (const void*)c->bank.desc;
  return FPC_OK;
}

int fpc_bank_destroy(fpc_ctx* c) {
  if (!c || !c->bank_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipStreamSynchronize(c->stream));                    // calls that still read the bank
  // the top-K workspace and the landmarks are sized by the bank: they go with it
  HIPCHECK(c->bank_slab.release());
  HIPCHECK(c->topk_slab.release());
  c->topk = BankTopkArgs{};
  HIPCHECK(c->pnp_topk_slab.release());
  c->pnp_topk_rec = nullptr; c->pnp_topk_np = nullptr; c->pnp_topk_best = nullptr;
  HIPCHECK(c->lm_slab.release());
  c->lm_xyzw = nullptr;
  c->bank = BankArgs{};
  c->bank_format = FPC_BANK_F32;
  c->bank16 = BankBf16Args{};
  return FPC_OK;
}

int fpc_bank_get(fpc_ctx* c, fpc_bank_view* out) {
  if (!c || !out || !c->bank_slab) return FPC_E_INVALID;
  out->desc = c->bank.desc;
  out->xy = c->bank.xy;
  out->count = c->bank.count;
  out->slots = c->bank.slots;
  out->rows = c->bank.rows;
  out->desc_dim = c->bank.D;
  out->chunk = c->bank.chunk;
  out->bytes = c->bank_slab.bytes;
  return FPC_OK;
}

// With a landmark reservation alive (fpc_bank_landmarks_reserve), whatever rewrites or empties a slot (-1: every slot)
// invalidates its landmarks: old points never attach to new rows.  Nothing is launched without a reservation.
static void landmarks_invalidate(fpc_ctx* c, int slot) {
  if (!c->lm_slab) return;
  hipLaunchKernelGGL(pnp_landmarks_invalidate_kernel, dim3((c->bank.rows + 255) / 256, slot < 0 ? c->bank.slots : 1), dim3(256),
                     0, c->stream, c->lm_xyzw, c->bank.rows, slot);
}

// the store kernel of the bank's format
static void bank_store_launch(fpc_ctx* c, int slot, const float* desc, const int32_t* xy, const int32_t* n, int src_cap) {
  const dim3 grid((c->bank.rows + 127) / 128);
  if (c->bank_format == FPC_BANK_BF16)
    hipLaunchKernelGGL(bank_store_bf16_kernel, grid, dim3(256), 0, c->stream, c->bank, c->bank16, slot, desc, xy, n, src_cap);
  else
    hipLaunchKernelGGL(bank_store_kernel, grid, dim3(256), 0, c->stream, c->bank, slot, desc, xy, n, src_cap);
  landmarks_invalidate(c, slot);
}

int fpc_bank_store(fpc_ctx* c, int frame, int slot) {
  if (!c || !c->bank_slab || !c->pts_desc || frame < 0 || frame >= c->pts_n || frame >= c->B || slot < 0 ||
      slot >= c->bank.slots)
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  bank_store_launch(c, slot, c->desc_out + (size_t)frame * c->cap * c->D, c->xy + (size_t)frame * c->cap * 2, c->count + frame,
                    c->cap);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_bank_store_rows(fpc_ctx* c, int slot, const float* desc, const int32_t* xy, const int32_t* n) {
  if (!c || !c->bank_slab || slot < 0 || slot >= c->bank.slots || !desc || !xy || !n ||
      (reinterpret_cast<uintptr_t>(desc) & 15))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  bank_store_launch(c, slot, desc, xy, n, c->bank.rows);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_bank_clear(fpc_ctx* c, int slot) {
  if (!c || !c->bank_slab || slot < -1 || slot >= c->bank.slots) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(bank_clear_kernel, dim3((c->bank.slots + 255) / 256), dim3(256), 0, c->stream, c->bank, slot);
  landmarks_invalidate(c, slot);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

// The bf16 kernels' instance for the context's descriptors: <8> k-steps of 16 at D = 128, <16> at D = 256.
extern "C++" template <typename K>      // (this block is extern "C")
static K by_depth(const fpc_ctx* c, K k8, K k16) { return c->D == 128 ? k8 : k16; }

// The bank as the train set of a (fp32 rows; a bf16 bank's kernels take theirs from c->bank16): frame f against slot[f].
static void bank_as_train(MatchFramesArgs& a, const BankArgs& b, const int32_t* slot) {
  a.key = b.desc; a.key_slot = slot; a.bank_norms = b.norms; a.bank_count = b.count;
  a.bank_rows = b.rows; a.bank_slots = b.slots;
}

// The score pass of fpc_match_bank and fpc_match_bank_topk, either format: the frames' norms (fp32: mf_norms_kernel, grid
// y = n, no key block; bf16: the rounding pass of match_bank_bf16.h, which writes the rounded rows too), then every (frame,
// slot) pair's strip and its count, the slots in chunks.  Leaves score [n][slots] in the bank's workspace; the norms (and
// rounded rows) stay valid for a table pass behind it.  D is 128 or 256.
static int bank_score_pass(fpc_ctx* c, const MatchFramesArgs& a, float max_dist, float ratio) {
  const BankArgs& b = c->bank;
  const BankBf16Args& h = c->bank16;
  const bool half = c->bank_format == FPC_BANK_BF16;
  const int n = a.n;
  const unsigned strips = (c->cap + MF_ROWS - 1) / MF_ROWS;
  if (half)
    hipLaunchKernelGGL(bank_round_queries_kernel, dim3((c->cap + 127) / 128, n), dim3(256), 0, c->stream, a, h);
  else
    hipLaunchKernelGGL(mf_norms_kernel, dim3((c->cap + 127) / 128, n), dim3(256), 0, c->stream, a);
  HIPCHECK(hipMemsetAsync(b.score, 0, sizeof(int32_t) * n * b.slots, c->stream));
  for (int s0 = 0; s0 < b.slots; s0 += b.chunk) {
    const int ns = std::min(b.chunk, b.slots - s0);
    if (a.cross_check)
      HIPCHECK(hipMemsetAsync(b.colbest, 0xff, sizeof(unsigned long long) * ((size_t)(n - 1) * b.chunk + ns) * b.rows, c->stream));
    if (half)
      hipLaunchKernelGGL(by_depth(c, bank_score_bf16_kernel<8>, bank_score_bf16_kernel<16>), dim3(strips, n, ns), dim3(256), 0,
                         c->stream, a, b, h, s0);
    else
      hipLaunchKernelGGL(bank_score_kernel, dim3(strips, n, ns), dim3(256), 0, c->stream, a, b, s0);
    hipLaunchKernelGGL(bank_count_kernel, dim3((c->cap + 255) / 256, n, ns), dim3(256), 0, c->stream, a, b, s0, max_dist, ratio);
  }
  return FPC_OK;
}

int fpc_match_bank(fpc_ctx* c, int n, int cross_check, float max_dist, float ratio, int min_score, int32_t* score,
                   int32_t* best, int32_t* match, float* dist) {
  if (!c || !c->bank_slab || (!score && !best) || !gate_ok(max_dist, ratio) || min_score < 0) return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, nullptr, nullptr)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const BankArgs& b = c->bank;
  MatchFramesArgs a = match_frames_args(c, n, nullptr, nullptr);
  a.cross_check = cross_check != 0;
  if (int rc = bank_score_pass(c, a, max_dist, ratio)) return rc;
  hipLaunchKernelGGL(bank_select_kernel, dim3(n), dim3(256), 0, c->stream, b, min_score, score, best);
  if (match || dist) {
    // the table of frame f against slot best[f]: fpc_match_frames' own kernels with a per-frame key; on a bf16 bank the
    // score pass's strip (match_bank_bf16.h), hence the same d^2 bits as the scores
    const dim3 strips((c->cap + MF_ROWS - 1) / MF_ROWS, n);
    bank_as_train(a, b, b.best);
    if (a.cross_check)
      HIPCHECK(hipMemsetAsync(c->mf_colbest, 0xff, sizeof(unsigned long long) * n * c->cap, c->stream));
    if (c->bank_format == FPC_BANK_BF16)
      hipLaunchKernelGGL(by_depth(c, match_bank_bf16_kernel<8, false>, match_bank_bf16_kernel<16, false>), strips, dim3(256), 0,
                         c->stream, a, b, c->bank16, MatchGuidedArgs{});
    else
      hipLaunchKernelGGL(match_frames_kernel, strips, dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(match_frames_finalize_kernel, dim3((c->cap + 255) / 256, n), dim3(256), 0, c->stream, a, max_dist,
                       ratio, match, dist);
  }
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_homography_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const fpc_ransac_params* p, float* H,
                        int32_t* ninliers, uint8_t* inlier) {
  if (!c || !H || !ninliers || !ransac_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_bank(c, a, n, slot, match, inlier)) return rc;
  return ransac_launch(c, a, H, ninliers, inlier, c->cap);
}

int fpc_fundamental_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const fpc_ransac_params* p, float* F,
                         int32_t* ninliers, uint8_t* inlier) {
  if (!c || !F || !ninliers || !ransac_params_ok(p, FM_SAMPLE)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n, p);
  if (int rc = pairs_bank(c, a, n, slot, match, inlier)) return rc;
  return fundamental_launch(c, a, F, ninliers, inlier, c->cap);
}

// ---- relative pose from a fundamental matrix (include/fpc.h; kernel in pose_epipolar.h) ------------------------------------
// The fundamental calls' pack / gather kernels with a NULL mask (nothing of the caller's is zeroed), their pair records and
// workspace: a pose call leaves the pair list its fundamental twin built, built again.
int fpc_default_pose_params(fpc_pose_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->reproj_threshold = 3.0f;
  p->min_front = 8;
  return FPC_OK;
}

static bool pose_params_ok(const fpc_pose_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         threshold_ok(p->reproj_threshold) && p->min_front >= 1;
}

// the solver step behind the pair list (a: hf_args with the parameters' threshold, nothing of RANSAC's)
static int pose_launch(fpc_ctx* c, const HfArgs& a, const fpc_pose_params* p, const float* F, float* R, float* t,
                       int32_t* nfront, float* xyz, uint8_t* front, int ostride) {
  const PoseArgs pa{p->q_fx, p->q_fy, p->q_cx, p->q_cy, p->t_fx, p->t_fy, p->t_cx, p->t_cy, p->min_front};
  hipLaunchKernelGGL(pose_kernel, dim3(a.n), dim3(256), 0, c->stream, a, pa, F, R, t, nfront, xyz, front, ostride);
  return launched();
}

int fpc_pose_fundamental(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                         const float* F, const fpc_pose_params* p, float* R, float* t, int32_t* nfront, float* xyz,
                         uint8_t* front) {
  if (!c || !F || !R || !t || !nfront || !pose_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, nullptr)) return rc;
  return pose_launch(c, a, p, F, R, t, nfront, xyz, front, stride);
}

int fpc_pose_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                    const float* F, const fpc_pose_params* p, float* R, float* t, int32_t* nfront, float* xyz,
                    uint8_t* front) {
  if (!c || !F || !R || !t || !nfront || !pose_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, nullptr)) return rc;
  return pose_launch(c, a, p, F, R, t, nfront, xyz, front, c->cap);
}

int fpc_pose_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const float* F, const fpc_pose_params* p,
                  float* R, float* t, int32_t* nfront, float* xyz, uint8_t* front) {
  if (!c || !F || !R || !t || !nfront || !pose_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_bank(c, a, n, slot, match, nullptr)) return rc;
  return pose_launch(c, a, p, F, R, t, nfront, xyz, front, c->cap);
}

// ---- relative pose from minimal samples: the 5-point essential matrix + 1 (include/fpc.h; kernels in essential_ransac.h) -----
// The fundamental calls' pack / gather kernels, pair records and workspace; the parameters are theirs and the pose calls'
// cameras, checked once for the three entry points.
int fpc_default_essential_params(fpc_essential_params* p) {
  if (!p) return FPC_E_INVALID;
  p->iterations = 1024;
  p->reproj_threshold = 3.0f;
  p->seed = 0;
  p->refits = 2;
  p->min_inliers = 8;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  return FPC_OK;
}

// the three calls' own checks (the pair source's follow in its helper), and their arguments on the pair-list workspace
static bool essential_ok(const fpc_ctx* c, const fpc_essential_params* p, const float* F, const int32_t* ninliers) {
  return c && F && ninliers && p && ransac_fields_ok(p->iterations, p->reproj_threshold, p->refits, p->min_inliers, ES_SAMPLE) &&
         camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy);
}
static EsArgs essential_args(const fpc_ctx* c, int n, const fpc_essential_params* p, int per_frame = 0) {
  EsArgs a{};
  static_cast<HfArgs&>(a) = hf_args(c, n, p->reproj_threshold, per_frame);
  a.T = p->iterations; a.refits = p->refits; a.min_inliers = p->min_inliers; a.seed = p->seed;
  a.q_fx = p->q_fx; a.q_fy = p->q_fy; a.q_cx = p->q_cx; a.q_cy = p->q_cy;
  a.t_fx = p->t_fx; a.t_fy = p->t_fy; a.t_cx = p->t_cx; a.t_cy = p->t_cy;
  return a;
}
static int essential_launch(fpc_ctx* c, const EsArgs& a, float* F, float* E, int32_t* ninliers, uint8_t* inlier, int mstride) {
  hipLaunchKernelGGL(essential_score_kernel, dim3((a.T + ES_THREADS - 1) / ES_THREADS, a.n), dim3(ES_THREADS), 0, c->stream, a);
  hipLaunchKernelGGL(essential_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, F, E, ninliers, inlier, mstride);
  return launched();
}

int fpc_ransac_essential(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                         const fpc_essential_params* p, float* F, float* E, int32_t* ninliers, uint8_t* inlier) {
  if (!essential_ok(c, p, F, ninliers)) return FPC_E_INVALID;
  const EsArgs a = essential_args(c, n, p);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, inlier)) return rc;
  return essential_launch(c, a, F, E, ninliers, inlier, stride);
}

int fpc_essential_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                         const fpc_essential_params* p, float* F, float* E, int32_t* ninliers, uint8_t* inlier) {
  if (!essential_ok(c, p, F, ninliers)) return FPC_E_INVALID;
  const EsArgs a = essential_args(c, n, p);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, inlier)) return rc;
  return essential_launch(c, a, F, E, ninliers, inlier, c->cap);
}

int fpc_essential_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const fpc_essential_params* p, float* F,
                       float* E, int32_t* ninliers, uint8_t* inlier) {
  if (!essential_ok(c, p, F, ninliers)) return FPC_E_INVALID;
  const EsArgs a = essential_args(c, n, p);
  if (int rc = pairs_bank(c, a, n, slot, match, inlier)) return rc;
  return essential_launch(c, a, F, E, ninliers, inlier, c->cap);
}

// ---- relative pose from a homography (include/fpc.h; kernel in pose_homography.h) ------------------------------------------
// The homography calls' pack / gather kernels with a NULL mask, their pair records and workspace, as the pose calls above.
int fpc_default_pose_homography_params(fpc_pose_homography_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->reproj_threshold = 3.0f;
  p->min_front = 8;
  p->min_baseline = 0.01f;
  p->which = 0;
  return FPC_OK;
}

static bool pose_homography_params_ok(const fpc_pose_homography_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         threshold_ok(p->reproj_threshold) && p->min_front >= 1 && std::isfinite(p->min_baseline) && p->min_baseline >= 0.f &&
         (p->which == 0 || p->which == 1);
}

// what the three calls share: the outputs that must exist
struct PoseHOut {
  int32_t* kind; float *R, *t, *plane; int32_t *nfront, *nplane; float* xyz; uint8_t* front;
  bool ok() const { return kind && R && t && nfront; }
};

// the solver step behind the pair list (a: hf_args with the parameters' threshold, nothing of RANSAC's)
static int pose_homography_launch(fpc_ctx* c, const HfArgs& a, const fpc_pose_homography_params* p, const float* H,
                                  const PoseHOut& o, int ostride) {
  const PoseHArgs pa{p->q_fx, p->q_fy, p->q_cx, p->q_cy, p->t_fx, p->t_fy, p->t_cx, p->t_cy, p->min_front, p->min_baseline,
                     p->which};
  hipLaunchKernelGGL(pose_homography_kernel, dim3(a.n), dim3(256), 0, c->stream, a, pa, H, o.kind, o.R, o.t, o.plane, o.nfront,
                     o.nplane, o.xyz, o.front, ostride);
  return launched();
}

int fpc_pose_homography(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                        const float* H, const fpc_pose_homography_params* p, int32_t* kind, float* R, float* t, float* plane,
                        int32_t* nfront, int32_t* nplane, float* xyz, uint8_t* front) {
  const PoseHOut o{kind, R, t, plane, nfront, nplane, xyz, front};
  if (!c || !H || !o.ok() || !pose_homography_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, nullptr)) return rc;
  return pose_homography_launch(c, a, p, H, o, stride);
}

int fpc_pose_homography_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                               const float* H, const fpc_pose_homography_params* p, int32_t* kind, float* R, float* t,
                               float* plane, int32_t* nfront, int32_t* nplane, float* xyz, uint8_t* front) {
  const PoseHOut o{kind, R, t, plane, nfront, nplane, xyz, front};
  if (!c || !H || !o.ok() || !pose_homography_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, nullptr)) return rc;
  return pose_homography_launch(c, a, p, H, o, c->cap);
}

int fpc_pose_homography_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const float* H,
                             const fpc_pose_homography_params* p, int32_t* kind, float* R, float* t, float* plane,
                             int32_t* nfront, int32_t* nplane, float* xyz, uint8_t* front) {
  const PoseHOut o{kind, R, t, plane, nfront, nplane, xyz, front};
  if (!c || !H || !o.ok() || !pose_homography_params_ok(p)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_bank(c, a, n, slot, match, nullptr)) return rc;
  return pose_homography_launch(c, a, p, H, o, c->cap);
}

// ---- absolute pose from bank landmarks: RANSAC PnP (include/fpc.h; kernels in pnp_ransac.h) ------------------------------------
int fpc_default_pnp_params(fpc_pnp_params* p) {
  if (!p) return FPC_E_INVALID;
  p->fx = p->fy = 500.0f;
  p->cx = 320.0f;
  p->cy = 240.0f;
  p->iterations = 1024;
  p->reproj_threshold = 3.0f;
  p->seed = 0;
  p->refits = 4;
  p->min_inliers = 12;
  return FPC_OK;
}

// the absolute-pose models share fpc_pnp_params; a model's sample size is its floor on min_inliers
enum PoseModel { POSE_DLT, POSE_P3P };
static bool pose_fields_ok(const fpc_pnp_params* p, int sample) {
  return p && camera_ok(p->fx, p->fy, p->cx, p->cy) &&
         ransac_fields_ok(p->iterations, p->reproj_threshold, p->refits, p->min_inliers, sample);
}
static bool pnp_params_ok(const fpc_pnp_params* p) { return pose_fields_ok(p, PNP_SAMPLE); }
static bool p3p_params_ok(const fpc_pnp_params* p) { return pose_fields_ok(p, P3P_SAMPLE); }
static bool pose_params_ok(const fpc_pnp_params* p, PoseModel model) {
  return model == POSE_P3P ? p3p_params_ok(p) : pnp_params_ok(p);
}

// The only PnP call that allocates or synchronises: pair records, counts and best keys of max_batch problems, an allocation
// of its own (the context slab, the plan hash, the bank's bytes and the RANSAC pair-list workspace are what they were).
int fpc_pnp_reserve(fpc_ctx* c, size_t* bytes) {
  if (!c || c->pnp_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  Carver cv(c);
  const size_t B = c->B, cap = c->cap;
  cv.into(&c->pnp_rec, B * cap * 2); cv.into(&c->pnp_np, B); cv.into(&c->pnp_best, B);
  if (int rc = c->pnp_slab.allocate(c->stream, cv)) return rc;
  if (bytes) *bytes = c->pnp_slab.bytes;
  return FPC_OK;
}

int fpc_bank_landmarks_reserve(fpc_ctx* c, size_t* bytes) {
  if (!c || !c->bank_slab || c->lm_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  Carver cv(c);
  cv.into(&c->lm_xyzw, (size_t)c->bank.slots * c->bank.rows);
  if (int rc = c->lm_slab.allocate(c->stream, cv)) return rc;           // (zeroed: no row is valid)
  if (bytes) *bytes = c->lm_slab.bytes;
  return FPC_OK;
}

int fpc_bank_store_landmarks(fpc_ctx* c, int slot, const float* xyz, const uint8_t* valid) {
  if (!c || !c->bank_slab || !c->lm_slab || slot < 0 || slot >= c->bank.slots || !xyz) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(pnp_landmarks_store_kernel, dim3((c->bank.rows + 255) / 256), dim3(256), 0, c->stream, c->lm_xyzw,
                     c->bank.count, c->bank.rows, slot, xyz, valid);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_bank_landmarks_get(fpc_ctx* c, const float** xyzw) {
  if (!c || !xyzw || !c->bank_slab || !c->lm_slab) return FPC_E_INVALID;
  *xyzw = reinterpret_cast<const float*>(c->lm_xyzw);
  return FPC_OK;
}

// A PnpArgs on the PnP reservation, one problem per frame; with per_frame = k on fpc_pnp_topk_reserve's, whose n problems are
// k per frame.
static PnpArgs pnp_args(fpc_ctx* c, int n, const fpc_pnp_params* p, int per_frame = 0) {
  PnpArgs a{};
  a.rec = per_frame ? c->pnp_topk_rec : c->pnp_rec; a.np = per_frame ? c->pnp_topk_np : c->pnp_np;
  a.best = per_frame ? c->pnp_topk_best : c->pnp_best;
  a.cap = c->cap; a.n = n; a.per_frame = per_frame;
  a.T = p->iterations; a.refits = p->refits; a.min_inliers = p->min_inliers;
  a.thr = p->reproj_threshold; a.seed = p->seed;
  a.fx = p->fx; a.fy = p->fy; a.cx = p->cx; a.cy = p->cy;
  return a;
}

// the solver step behind the pair list: the model's score kernel and its refit kernel
static int pnp_launch(fpc_ctx* c, PoseModel model, const PnpArgs& a, float* R, float* t, int32_t* ninliers, uint8_t* inlier,
                      int mstride) {
  if (model == POSE_P3P) {
    hipLaunchKernelGGL(p3p_score_kernel, dim3((a.T + P3P_THREADS - 1) / P3P_THREADS, a.n), dim3(P3P_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(p3p_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, R, t, ninliers, inlier, mstride);
  } else {
    hipLaunchKernelGGL(pnp_score_kernel, dim3((a.T + PNP_THREADS - 1) / PNP_THREADS, a.n), dim3(PNP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(pnp_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, R, t, ninliers, inlier, mstride);
  }
  return launched();
}

// fpc_pnp_frames / fpc_pnp_bank and their P3P twins: the gather kernel over either train set, then the model's solver
// (a: pnp_args; its a.n problems are the frames, or per_frame of them each -- the top-K calls, whose tr.slot and match hold
// an entry per problem)
static int pnp_gather(fpc_ctx* c, PoseModel model, const PnpArgs& a, const PnpTrain& tr, const int32_t* match, float* R, float* t,
                      int32_t* ninliers, uint8_t* inlier) {
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(pnp_gather_kernel, dim3(a.n), dim3(256), 0, c->stream, a, c->xy, c->count, match, inlier, tr);
  return pnp_launch(c, model, a, R, t, ninliers, inlier, c->cap);
}

// The three pair sources, each written once for both models: the checks, the pair list, the solver.
static int pose_explicit(fpc_ctx* c, PoseModel model, int n, const float* xy, const float* xyz, const int32_t* npairs, int stride,
                         const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !xy || !xyz || !npairs || !R || !t || !ninliers || !pose_params_ok(p, model) ||
      !explicit_ok(c, n, stride))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const PnpArgs a = pnp_args(c, n, p);
  hipLaunchKernelGGL(pnp_pack_kernel, dim3((stride + 255) / 256, n), dim3(256), 0, c->stream, a, xy, xyz, npairs, stride, inlier);
  return pnp_launch(c, model, a, R, t, ninliers, inlier, stride);
}

static int pose_frames(fpc_ctx* c, PoseModel model, int n, const float* key_xyz, const uint8_t* key_valid, const int32_t* nkey,
                       const int32_t* match, const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !key_xyz || !nkey || !match || !R || !t || !ninliers || !pose_params_ok(p, model) || !frames_ok(c, n))
    return FPC_E_INVALID;
  return pnp_gather(c, model, pnp_args(c, n, p), PnpTrain{key_xyz, key_valid, nkey, nullptr, nullptr, nullptr, 0, 0}, match, R, t,
                    ninliers, inlier);
}

static int pose_bank(fpc_ctx* c, PoseModel model, int n, const int32_t* slot, const int32_t* match, const fpc_pnp_params* p,
                     float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !R || !t || !ninliers || !pose_params_ok(p, model) || !bank_ok(c, n, slot, match))
    return FPC_E_INVALID;
  // (without landmark storage lm is null: no frame has pairs)
  return pnp_gather(c, model, pnp_args(c, n, p),
                    PnpTrain{nullptr, nullptr, nullptr, slot, c->lm_xyzw, c->bank.count, c->bank.rows, c->bank.slots}, match, R, t,
                    ninliers, inlier);
}

int fpc_ransac_pnp(fpc_ctx* c, int n, const float* xy, const float* xyz, const int32_t* npairs, int stride,
                   const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  return pose_explicit(c, POSE_DLT, n, xy, xyz, npairs, stride, p, R, t, ninliers, inlier);
}

int fpc_pnp_frames(fpc_ctx* c, int n, const float* key_xyz, const uint8_t* key_valid, const int32_t* nkey, const int32_t* match,
                   const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  return pose_frames(c, POSE_DLT, n, key_xyz, key_valid, nkey, match, p, R, t, ninliers, inlier);
}

int fpc_pnp_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const fpc_pnp_params* p, float* R, float* t,
                 int32_t* ninliers, uint8_t* inlier) {
  return pose_bank(c, POSE_DLT, n, slot, match, p, R, t, ninliers, inlier);
}

// ---- absolute pose from a minimal sample: P3P + 1 (include/fpc.h; kernels in p3p_ransac.h) -----------------------------------
int fpc_ransac_p3p(fpc_ctx* c, int n, const float* xy, const float* xyz, const int32_t* npairs, int stride,
                   const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  return pose_explicit(c, POSE_P3P, n, xy, xyz, npairs, stride, p, R, t, ninliers, inlier);
}

int fpc_p3p_frames(fpc_ctx* c, int n, const float* key_xyz, const uint8_t* key_valid, const int32_t* nkey, const int32_t* match,
                   const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  return pose_frames(c, POSE_P3P, n, key_xyz, key_valid, nkey, match, p, R, t, ninliers, inlier);
}

int fpc_p3p_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const fpc_pnp_params* p, float* R, float* t,
                 int32_t* ninliers, uint8_t* inlier) {
  return pose_bank(c, POSE_P3P, n, slot, match, p, R, t, ninliers, inlier);
}

// ---- Sim(3) alignment between two frames' landmarks (include/fpc.h; kernels in sim3_ransac.h) ----------------------------------
int fpc_default_sim3_params(fpc_sim3_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->iterations = 1024;
  p->reproj_threshold = 3.0f;
  p->seed = 0;
  p->refits = 4;
  p->min_inliers = 12;
  p->fix_scale = 0;
  return FPC_OK;
}

static bool sim3_params_ok(const fpc_sim3_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         ransac_fields_ok(p->iterations, p->reproj_threshold, p->refits, p->min_inliers, SIM3_SAMPLE) &&
         (p->fix_scale == 0 || p->fix_scale == 1);
}

// the records, counts and best keys are the PnP reservation's (the records have the PnP records' size)
static Sim3Args sim3_args(fpc_ctx* c, int n, const fpc_sim3_params* p) {
  Sim3Args a{};
  a.rec = c->pnp_rec; a.np = c->pnp_np; a.best = c->pnp_best;
  a.cap = c->cap; a.n = n;
  a.T = p->iterations; a.refits = p->refits; a.min_inliers = p->min_inliers; a.fix_scale = p->fix_scale;
  a.thr = p->reproj_threshold; a.seed = p->seed;
  a.qfx = p->q_fx; a.qfy = p->q_fy; a.tfx = p->t_fx; a.tfy = p->t_fy;
  return a;
}

// the solver step behind the pair list
static int sim3_launch(fpc_ctx* c, const Sim3Args& a, float* s, float* R, float* t, int32_t* ninliers, uint8_t* inlier,
                       int mstride) {
  hipLaunchKernelGGL(sim3_score_kernel, dim3((a.T + SIM3_THREADS - 1) / SIM3_THREADS, a.n), dim3(SIM3_THREADS), 0, c->stream, a);
  hipLaunchKernelGGL(sim3_refit_kernel, dim3(a.n), dim3(256), 0, c->stream, a, s, R, t, ninliers, inlier, mstride);
  return launched();
}

// fpc_sim3_frames / fpc_sim3_bank: the gather kernel over either train set, then the solver
static int sim3_gather(fpc_ctx* c, int n, const float* q_xyz, const uint8_t* q_valid, const PnpTrain& tr, const int32_t* match,
                       const fpc_sim3_params* p, float* s, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  HIPCHECK(hipSetDevice(c->cfg.device));
  const Sim3Args a = sim3_args(c, n, p);
  hipLaunchKernelGGL(sim3_gather_kernel, dim3(n), dim3(256), 0, c->stream, a, q_xyz, q_valid, c->count, match, inlier, tr);
  return sim3_launch(c, a, s, R, t, ninliers, inlier, c->cap);
}

int fpc_ransac_sim3(fpc_ctx* c, int n, const float* q_xyz, const float* t_xyz, const int32_t* npairs, int stride,
                    const fpc_sim3_params* p, float* s, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !q_xyz || !t_xyz || !npairs || !s || !R || !t || !ninliers || !sim3_params_ok(p) ||
      !explicit_ok(c, n, stride))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const Sim3Args a = sim3_args(c, n, p);
  hipLaunchKernelGGL(sim3_pack_kernel, dim3((stride + 255) / 256, n), dim3(256), 0, c->stream, a, q_xyz, t_xyz, npairs, stride,
                     inlier);
  return sim3_launch(c, a, s, R, t, ninliers, inlier, stride);
}

int fpc_sim3_frames(fpc_ctx* c, int n, const float* q_xyz, const uint8_t* q_valid, const float* key_xyz, const uint8_t* key_valid,
                    const int32_t* nkey, const int32_t* match, const fpc_sim3_params* p, float* s, float* R, float* t,
                    int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !q_xyz || !key_xyz || !nkey || !match || !s || !R || !t || !ninliers || !sim3_params_ok(p) ||
      !frames_ok(c, n))
    return FPC_E_INVALID;
  return sim3_gather(c, n, q_xyz, q_valid, PnpTrain{key_xyz, key_valid, nkey, nullptr, nullptr, nullptr, 0, 0}, match, p, s, R,
                     t, ninliers, inlier);
}

int fpc_sim3_bank(fpc_ctx* c, int n, const float* q_xyz, const uint8_t* q_valid, const int32_t* slot, const int32_t* match,
                  const fpc_sim3_params* p, float* s, float* R, float* t, int32_t* ninliers, uint8_t* inlier) {
  if (!c || !c->pnp_slab || !q_xyz || !s || !R || !t || !ninliers || !sim3_params_ok(p) || !bank_ok(c, n, slot, match))
    return FPC_E_INVALID;
  // (without landmark storage lm is null: no frame has pairs)
  return sim3_gather(c, n, q_xyz, q_valid,
                     PnpTrain{nullptr, nullptr, nullptr, slot, c->lm_xyzw, c->bank.count, c->bank.rows, c->bank.slots}, match, p,
                     s, R, t, ninliers, inlier);
}

// ---- top-K candidates of the bank, each verified by RANSAC (include/fpc.h; kernels in match_bank_topk.h) -------------------
// The only call of the three that allocates or synchronises: pair tables and RANSAC workspace for max_batch x kmax (frame,
// candidate) pairs, an allocation of its own (the bank's bytes / chunk and the context slab are what they were).
int fpc_bank_topk_reserve(fpc_ctx* c, int kmax, size_t* bytes) {
  if (!c || !c->bank_slab || c->topk_slab || kmax < 1 || kmax > std::min((int)FPC_BANK_TOPK_MAX, c->bank.slots))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t pairs = (size_t)c->B * kmax, cap = c->cap, rows = c->bank.rows;
  Carver cv(c);
  cv.into(&c->topk.top2, pairs * cap * 2); cv.into(&c->topk.colbest, pairs * rows);
  cv.into(&c->topk.cand_slot, pairs); cv.into(&c->topk.cand_score, pairs);
  cv.into(&c->topk_pairs, pairs * cap); cv.into(&c->topk_row, pairs * cap);
  cv.into(&c->topk_np, pairs); cv.into(&c->topk_best, pairs);
  if (int rc = c->topk_slab.allocate(c->stream, cv)) return rc;
  c->topk.kmax = kmax;
  if (bytes) *bytes = c->topk_slab.bytes;
  return FPC_OK;
}

int fpc_match_bank_topk(fpc_ctx* c, int n, int k, int cross_check, float max_dist, float ratio, int min_score, int32_t* score,
                        int32_t* cand_slot, int32_t* cand_score, int32_t* match, float* dist) {
  if (!c || !c->bank_slab || !c->topk_slab || !cand_slot || k < 1 || k > c->topk.kmax || !gate_ok(max_dist, ratio) ||
      min_score < 0)
    return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, nullptr, nullptr)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const BankArgs& b = c->bank;
  const BankTopkArgs& t = c->topk;
  MatchFramesArgs a = match_frames_args(c, n, nullptr, nullptr);
  a.cross_check = cross_check != 0;
  if (int rc = bank_score_pass(c, a, max_dist, ratio)) return rc;
  hipLaunchKernelGGL(bank_topk_kernel, dim3(n), dim3(256), 0, c->stream, b, t, k, min_score, score, cand_slot, cand_score);
  if (match || dist) {
    // the k tables of every frame in one launch: the score pass's strip against slot cand_slot[f][z] (the norms, and on a
    // bf16 bank the rounded query rows, are the score pass's)
    const dim3 strips((c->cap + MF_ROWS - 1) / MF_ROWS, n, k);
    if (a.cross_check)
      HIPCHECK(hipMemsetAsync(t.colbest, 0xff, sizeof(unsigned long long) * ((size_t)(n - 1) * t.kmax + k) * b.rows, c->stream));
    if (c->bank_format == FPC_BANK_BF16)
      hipLaunchKernelGGL(by_depth(c, bank_topk_table_bf16_kernel<8>, bank_topk_table_bf16_kernel<16>), strips, dim3(256), 0,
                         c->stream, a, b, c->bank16, t);
    else
      hipLaunchKernelGGL(bank_topk_table_kernel, strips, dim3(256), 0, c->stream, a, b, t);
    hipLaunchKernelGGL(bank_topk_finalize_kernel, dim3((c->cap + 255) / 256, n, k), dim3(256), 0, c->stream, a, b, t, k,
                       max_dist, ratio, match, dist);
  }
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

int fpc_homography_bank_topk(fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match,
                             const fpc_ransac_params* p, float* H, int32_t* ninliers, uint8_t* inlier, int32_t* pick,
                             int32_t* best) {
  if (!c || !H || !ninliers || !ransac_params_ok(p) || !c->topk_slab || k < 1 || k > c->topk.kmax || !frames_ok(c, n))
    return FPC_E_INVALID;
  // n k problems on the reserved workspace: problem f k + j is frame f against slot cand_slot[f][j] with match[f][j]
  const HfArgs a = ransac_args(c, n * k, p, k);
  if (int rc = pairs_bank(c, a, n, cand_slot, match, inlier)) return rc;
  if (int rc = ransac_launch(c, a, H, ninliers, inlier, c->cap)) return rc;
  if (pick || best)
    hipLaunchKernelGGL(bank_pick_kernel, dim3(n), dim3(64), 0, c->stream, ninliers, cand_slot, k, pick, best);
  return launched();
}

// ---- top-K candidates under the pose and epipolar models (include/fpc.h): the single-slot bank calls' kernels over n k
// ---- problems (per_frame = k), then the pick and the picked candidate's model -------------------------------------------------
// what the four calls refuse beside their single-slot twins' checks
static bool topk_ok(const fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match) {
  return c->topk_slab && k >= 1 && k <= c->topk.kmax && bank_ok(c, n, cand_slot, match);
}
// their tail: m0 [n][k][w0] (R or F) and m1 [n][k][w1] (t, or null) -> best0 [n][w0], best1 [n][w1]
static int topk_pick(fpc_ctx* c, int n, int k, const int32_t* ninliers, const int32_t* cand_slot, int32_t* pick, int32_t* best,
                     const float* m0, int w0, float* best0, const float* m1, int w1, float* best1) {
  if (pick || best || best0 || best1)
    hipLaunchKernelGGL(bank_pick_model_kernel, dim3(n), dim3(64), 0, c->stream, ninliers, cand_slot, k, pick, best, m0, w0, best0,
                       m1, w1, best1);
  return launched();
}

// The only call of the pose top-K calls that allocates or synchronises: the PnP reservation's three buffers for max_batch x
// kmax problems, an allocation of its own (the bank's bytes, the top-K reservation and the PnP reservation are what they were).
int fpc_pnp_topk_reserve(fpc_ctx* c, size_t* bytes) {
  if (!c || !c->bank_slab || !c->topk_slab || c->pnp_topk_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t problems = (size_t)c->B * c->topk.kmax, cap = c->cap;
  Carver cv(c);
  cv.into(&c->pnp_topk_rec, problems * cap * 2); cv.into(&c->pnp_topk_np, problems); cv.into(&c->pnp_topk_best, problems);
  if (int rc = c->pnp_topk_slab.allocate(c->stream, cv)) return rc;
  if (bytes) *bytes = c->pnp_topk_slab.bytes;
  return FPC_OK;
}

static int pose_bank_topk(fpc_ctx* c, PoseModel model, int n, int k, const int32_t* cand_slot, const int32_t* match,
                          const fpc_pnp_params* p, float* R, float* t, int32_t* ninliers, uint8_t* inlier, int32_t* pick,
                          int32_t* best, float* best_R, float* best_t) {
  if (!c || !c->pnp_topk_slab || !R || !t || !ninliers || !pose_params_ok(p, model) || !topk_ok(c, n, k, cand_slot, match))
    return FPC_E_INVALID;
  // n k problems on the reserved records: problem f k + j is frame f against the landmarks of slot cand_slot[f][j] with
  // match[f][j] (without landmark storage lm is null: no problem has pairs)
  if (int rc = pnp_gather(c, model, pnp_args(c, n * k, p, k),
                          PnpTrain{nullptr, nullptr, nullptr, cand_slot, c->lm_xyzw, c->bank.count, c->bank.rows, c->bank.slots},
                          match, R, t, ninliers, inlier))
    return rc;
  return topk_pick(c, n, k, ninliers, cand_slot, pick, best, R, 9, best_R, t, 3, best_t);
}

int fpc_pnp_bank_topk(fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match, const fpc_pnp_params* p, float* R,
                      float* t, int32_t* ninliers, uint8_t* inlier, int32_t* pick, int32_t* best, float* best_R, float* best_t) {
  return pose_bank_topk(c, POSE_DLT, n, k, cand_slot, match, p, R, t, ninliers, inlier, pick, best, best_R, best_t);
}

int fpc_p3p_bank_topk(fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match, const fpc_pnp_params* p, float* R,
                      float* t, int32_t* ninliers, uint8_t* inlier, int32_t* pick, int32_t* best, float* best_R, float* best_t) {
  return pose_bank_topk(c, POSE_P3P, n, k, cand_slot, match, p, R, t, ninliers, inlier, pick, best, best_R, best_t);
}

int fpc_fundamental_bank_topk(fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match,
                              const fpc_ransac_params* p, float* F, int32_t* ninliers, uint8_t* inlier, int32_t* pick,
                              int32_t* best, float* best_F) {
  if (!c || !F || !ninliers || !ransac_params_ok(p, FM_SAMPLE) || !topk_ok(c, n, k, cand_slot, match)) return FPC_E_INVALID;
  const HfArgs a = ransac_args(c, n * k, p, k);
  if (int rc = pairs_bank(c, a, n, cand_slot, match, inlier)) return rc;
  if (int rc = fundamental_launch(c, a, F, ninliers, inlier, c->cap)) return rc;
  return topk_pick(c, n, k, ninliers, cand_slot, pick, best, F, 9, best_F, nullptr, 0, nullptr);
}

int fpc_essential_bank_topk(fpc_ctx* c, int n, int k, const int32_t* cand_slot, const int32_t* match,
                            const fpc_essential_params* p, float* F, float* E, int32_t* ninliers, uint8_t* inlier, int32_t* pick,
                            int32_t* best, float* best_F) {
  if (!essential_ok(c, p, F, ninliers) || !topk_ok(c, n, k, cand_slot, match)) return FPC_E_INVALID;
  const EsArgs a = essential_args(c, n * k, p, k);
  if (int rc = pairs_bank(c, a, n, cand_slot, match, inlier)) return rc;
  if (int rc = essential_launch(c, a, F, E, ninliers, inlier, c->cap)) return rc;
  return topk_pick(c, n, k, ninliers, cand_slot, pick, best, F, 9, best_F, nullptr, 0, nullptr);
}

// ---- guided matching: plain, cell-ordered, epipolar and under a pose (include/fpc.h; two strip skeletons and three gates in
// ---- match_guided.h, match_guided_cells.h, match_guided_epipolar.h and match_guided_pose.h, five kernels) -----------------------
// 32-px cells wherever the order is public; a frame of more cells than the order kernel's histogram holds (beyond
// 16.7 MPx) is ordered in coarser cells by the guided calls, whose output does not depend on the order.
static CellOrderArgs cell_order_args(fpc_ctx* c, int shift) {
  CellOrderArgs o{};
  o.shift = shift;
  o.CX = (c->W + (1 << shift) - 1) >> shift;
  o.CY = (c->H + (1 << shift) - 1) >> shift;
  return o;
}

int fpc_cell_order(fpc_ctx* c, const int32_t* xy, const int32_t* n, int sets, int stride, int32_t* perm) {
  if (!c || !xy || !n || !perm || sets < 1 || stride < 1) return FPC_E_INVALID;
  CellOrderArgs o = cell_order_args(c, 5);
  if ((long long)o.CX * o.CY > MGC_MAX_CELLS) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  o.xy = xy; o.n = n; o.stride = o.out_stride = stride; o.perm = perm;
  hipLaunchKernelGGL(cell_order_kernel, dim3(sets), dim3(256), 0, c->stream, o);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

// The order passes in front of match_guided_cells_kernel / match_guided_epipolar_cells_kernel: the frames' rows, then the
// train sets -- the key once, the bank's slot of every frame (a.key_slot), none under FPC_PAIR_PREVIOUS without a key
// (frame f - 1's query order).
static MatchCellsArgs cell_order_passes(fpc_ctx* c, const MatchFramesArgs& a, const MatchGuidedArgs& g, int32_t* stats) {
  const int nbox = (c->cap + 63) / 64;
  int shift = 5;
  while ((long long)((c->W + (1 << shift) - 1) >> shift) * ((c->H + (1 << shift) - 1) >> shift) > MGC_MAX_CELLS) ++shift;
  CellOrderArgs o = cell_order_args(c, shift);
  o.xy = c->xy; o.n = c->count; o.stride = o.out_stride = c->cap;
  o.perm = c->mgc_perm_q; o.box = c->mgc_box; o.box_stride = nbox;
  hipLaunchKernelGGL(cell_order_kernel, dim3(a.n), dim3(256), 0, c->stream, o);
  int4* box_t = c->mgc_box + (size_t)c->B * nbox;
  if (a.key_slot || a.key) {
    CellOrderArgs t = cell_order_args(c, shift);
    t.xy = g.key_xy; t.out_stride = c->cap; t.perm = c->mgc_perm_t; t.box = box_t; t.box_stride = nbox;
    if (a.key_slot) {
      t.n = a.bank_count; t.slot = a.key_slot; t.nslots = a.bank_slots; t.stride = a.bank_rows;
    } else {
      t.n = a.nkey; t.stride = c->cap;
    }
    hipLaunchKernelGGL(cell_order_kernel, dim3(a.key_slot ? a.n : 1), dim3(256), 0, c->stream, t);
  }
  return MatchCellsArgs{c->mgc_perm_q, c->mgc_box, c->mgc_perm_t, box_t, nbox, stats};
}

// The ten guided entry points run on fpc_match_frames' workspace (norms, top-2, column minima: [max_batch][cap], and the
// bank's rows <= cap), carved at fpc_create: nothing of their own.  One sequence for all: the column minima and the stats
// reset, the norms (a bf16 bank: its rounding pass, match_bank_bf16.h), the variant's strip kernel (the four fp32 ones are
// mg_strip / mgc_strip with the homography or the epipolar gate; the cell-ordered ones run behind their order passes; the
// pose strip is mg_strip with the pose gate and takes its own arguments, `pose`, in place of g), the finalize kernel.
// norm_blocks: n + 1 with the key's block, n against the bank, whose norms are its own.
enum GuidedStrip { GUIDED_PLAIN, GUIDED_CELLS, GUIDED_BANK_BF16, GUIDED_EPIPOLAR, GUIDED_EPIPOLAR_CELLS, GUIDED_POSE };

static int match_guided_launch(fpc_ctx* c, GuidedStrip strip, MatchFramesArgs a, const MatchGuidedArgs& g, int norm_blocks,
                               float max_dist, float ratio, int32_t* match, float* dist, int32_t* stats,
                               const MatchPoseArgs* pose = nullptr) {
  const dim3 norms((c->cap + 127) / 128, norm_blocks), strips((c->cap + MF_ROWS - 1) / MF_ROWS, a.n);
  if (a.cross_check)
    HIPCHECK(hipMemsetAsync(c->mf_colbest, 0xff, sizeof(unsigned long long) * a.n * c->cap, c->stream));
  if (stats) HIPCHECK(hipMemsetAsync(stats, 0, sizeof(int32_t) * 2 * a.n, c->stream));
  if (strip == GUIDED_BANK_BF16)
    hipLaunchKernelGGL(bank_round_queries_kernel, norms, dim3(256), 0, c->stream, a, c->bank16);
  else
    hipLaunchKernelGGL(mf_norms_kernel, norms, dim3(256), 0, c->stream, a);
  if (strip == GUIDED_CELLS) {
    const MatchCellsArgs m = cell_order_passes(c, a, g, stats);
    hipLaunchKernelGGL(match_guided_cells_kernel, strips, dim3(256), 0, c->stream, a, g, m);
  } else if (strip == GUIDED_BANK_BF16) {
    hipLaunchKernelGGL(by_depth(c, match_bank_bf16_kernel<8, true>, match_bank_bf16_kernel<16, true>), strips, dim3(256), 0,
                       c->stream, a, c->bank, c->bank16, g);
  } else if (strip == GUIDED_EPIPOLAR_CELLS) {
    const MatchCellsArgs m = cell_order_passes(c, a, g, stats);
    hipLaunchKernelGGL(match_guided_epipolar_cells_kernel, strips, dim3(256), 0, c->stream, a, g, m);     // (g.H holds F)
  } else if (strip == GUIDED_EPIPOLAR) {
    hipLaunchKernelGGL(match_guided_epipolar_kernel, strips, dim3(256), 0, c->stream, a, g);     // (g.H holds F)
  } else if (strip == GUIDED_POSE) {
    hipLaunchKernelGGL(match_guided_pose_kernel, strips, dim3(256), 0, c->stream, a, *pose);
  } else {
    hipLaunchKernelGGL(match_guided_kernel, strips, dim3(256), 0, c->stream, a, g);
  }
  hipLaunchKernelGGL(match_guided_finalize_kernel, dim3((c->cap + 255) / 256, a.n), dim3(256), 0, c->stream, a, max_dist,
                     ratio, match, dist);
  HIPCHECK(hipGetLastError());
  return FPC_OK;
}

static bool guided_options_ok(const float* H, float radius, float max_dist, float ratio, const int32_t* match) {
  return H && match && std::isfinite(radius) && radius > 0.f && gate_ok(max_dist, ratio);
}

// fpc_match_frames_guided[_cells | _epipolar | _epipolar_cells]: the key set (or frame f - 1) as the train set
static int match_frames_guided(fpc_ctx* c, GuidedStrip strip, int n, int pairing, const float* key, const int32_t* nkey,
                               const int32_t* key_xy, const float* H, float radius, int cross_check, float max_dist,
                               float ratio, int32_t* match, float* dist, int32_t* stats) {
  if (!c || !guided_options_ok(H, radius, max_dist, ratio, match) || !pairing_ok(pairing) ||
      (pairing == FPC_PAIR_KEY && (!key || !key_xy)) || (key && !key_xy))
    return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, key, nkey)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, key, nkey);
  a.pairing = pairing;
  a.cross_check = cross_check != 0;
  const MatchGuidedArgs g{H, c->xy, key ? key_xy : nullptr, (double)radius * (double)radius};
  return match_guided_launch(c, strip, a, g, n + 1, max_dist, ratio, match, dist, stats);
}

// fpc_match_bank_guided[_cells | _epipolar | _epipolar_cells]: bank slot slot[f] as frame f's train set (strip: GUIDED_PLAIN
// stands for the bank's own format, fp32 or bf16)
static int match_bank_guided(fpc_ctx* c, GuidedStrip strip, int n, const int32_t* slot, const float* H, float radius, int cross_check,
                             float max_dist, float ratio, int32_t* match, float* dist, int32_t* stats) {
  if (!c || !c->bank_slab || !slot || !guided_options_ok(H, radius, max_dist, ratio, match)) return FPC_E_INVALID;
  const bool half = c->bank_format != FPC_BANK_F32;
  if (strip != GUIDED_PLAIN && half) return FPC_E_INVALID;     // (the bf16 bank's ordered and epipolar strips: not built yet)
  if (int rc = match_frames_check(c, n, nullptr, nullptr)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, nullptr, nullptr);
  a.cross_check = cross_check != 0;
  bank_as_train(a, c->bank, slot);
  const MatchGuidedArgs g{H, c->xy, c->bank.xy, (double)radius * (double)radius};
  return match_guided_launch(c, half ? GUIDED_BANK_BF16 : strip, a, g, n, max_dist, ratio, match, dist, stats);
}

int fpc_match_frames_guided(fpc_ctx* c, int n, int pairing, const float* key, const int32_t* nkey, const int32_t* key_xy,
                            const float* H, float radius, int cross_check, float max_dist, float ratio, int32_t* match,
                            float* dist) {
  return match_frames_guided(c, GUIDED_PLAIN, n, pairing, key, nkey, key_xy, H, radius, cross_check, max_dist, ratio, match, dist,
                             nullptr);
}

int fpc_match_frames_guided_cells(fpc_ctx* c, int n, int pairing, const float* key, const int32_t* nkey,
                                  const int32_t* key_xy, const float* H, float radius, int cross_check, float max_dist,
                                  float ratio, int32_t* match, float* dist, int32_t* stats) {
  return match_frames_guided(c, GUIDED_CELLS, n, pairing, key, nkey, key_xy, H, radius, cross_check, max_dist, ratio, match, dist,
                             stats);
}

int fpc_match_bank_guided(fpc_ctx* c, int n, const int32_t* slot, const float* H, float radius, int cross_check,
                          float max_dist, float ratio, int32_t* match, float* dist) {
  return match_bank_guided(c, GUIDED_PLAIN, n, slot, H, radius, cross_check, max_dist, ratio, match, dist, nullptr);
}

int fpc_match_bank_guided_cells(fpc_ctx* c, int n, const int32_t* slot, const float* H, float radius, int cross_check,
                                float max_dist, float ratio, int32_t* match, float* dist, int32_t* stats) {
  return match_bank_guided(c, GUIDED_CELLS, n, slot, H, radius, cross_check, max_dist, ratio, match, dist, stats);
}

int fpc_match_frames_guided_epipolar(fpc_ctx* c, int n, int pairing, const float* key, const int32_t* nkey,
                                     const int32_t* key_xy, const float* F, float radius, int cross_check, float max_dist,
                                     float ratio, int32_t* match, float* dist) {
  return match_frames_guided(c, GUIDED_EPIPOLAR, n, pairing, key, nkey, key_xy, F, radius, cross_check, max_dist, ratio, match,
                             dist, nullptr);
}

int fpc_match_bank_guided_epipolar(fpc_ctx* c, int n, const int32_t* slot, const float* F, float radius, int cross_check,
                                   float max_dist, float ratio, int32_t* match, float* dist) {
  return match_bank_guided(c, GUIDED_EPIPOLAR, n, slot, F, radius, cross_check, max_dist, ratio, match, dist, nullptr);
}

int fpc_match_frames_guided_epipolar_cells(fpc_ctx* c, int n, int pairing, const float* key, const int32_t* nkey,
                                           const int32_t* key_xy, const float* F, float radius, int cross_check,
                                           float max_dist, float ratio, int32_t* match, float* dist, int32_t* stats) {
  return match_frames_guided(c, GUIDED_EPIPOLAR_CELLS, n, pairing, key, nkey, key_xy, F, radius, cross_check, max_dist, ratio,
                             match, dist, stats);
}

int fpc_match_bank_guided_epipolar_cells(fpc_ctx* c, int n, const int32_t* slot, const float* F, float radius, int cross_check,
                                         float max_dist, float ratio, int32_t* match, float* dist, int32_t* stats) {
  return match_bank_guided(c, GUIDED_EPIPOLAR_CELLS, n, slot, F, radius, cross_check, max_dist, ratio, match, dist, stats);
}

// fpc_match_frames_guided_pose / fpc_match_bank_guided_pose: the gate reads the train set's landmarks -- the key's, or the
// bank's (null without a landmark reservation: no row is valid) -- and no train pixels
static bool pose_options_ok(const float* R, const float* t, float fx, float fy, float cx, float cy, float radius,
                            float max_dist, float ratio, const int32_t* match) {
  return t && guided_options_ok(R, radius, max_dist, ratio, match) && camera_ok(fx, fy, cx, cy);
}

static MatchPoseArgs match_pose_args(fpc_ctx* c, const float* R, const float* t, float fx, float fy, float cx, float cy,
                                     float radius) {
  MatchPoseArgs g{};
  g.R = R; g.t = t; g.xy = c->xy;
  g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
  g.r2 = (double)radius * (double)radius;
  return g;
}

int fpc_match_frames_guided_pose(fpc_ctx* c, int n, const float* key, const int32_t* nkey, const float* key_xyz,
                                 const uint8_t* key_valid, const float* R, const float* t, float fx, float fy, float cx,
                                 float cy, float radius, int cross_check, float max_dist, float ratio, int32_t* match,
                                 float* dist) {
  if (!c || !key || !nkey || !key_xyz || !pose_options_ok(R, t, fx, fy, cx, cy, radius, max_dist, ratio, match))
    return FPC_E_INVALID;
  if (int rc = match_frames_check(c, n, key, nkey)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, key, nkey);
  a.pairing = FPC_PAIR_KEY;
  a.cross_check = cross_check != 0;
  MatchPoseArgs g = match_pose_args(c, R, t, fx, fy, cx, cy, radius);
  g.key_xyz = key_xyz; g.key_valid = key_valid;
  return match_guided_launch(c, GUIDED_POSE, a, MatchGuidedArgs{}, n + 1, max_dist, ratio, match, dist, nullptr, &g);
}

int fpc_match_bank_guided_pose(fpc_ctx* c, int n, const int32_t* slot, const float* R, const float* t, float fx, float fy,
                               float cx, float cy, float radius, int cross_check, float max_dist, float ratio, int32_t* match,
                               float* dist) {
  if (!c || !c->bank_slab || !slot || !pose_options_ok(R, t, fx, fy, cx, cy, radius, max_dist, ratio, match))
    return FPC_E_INVALID;
  if (c->bank_format != FPC_BANK_F32) return FPC_E_INVALID;     // (the bf16 bank's pose gate: not built yet)
  if (int rc = match_frames_check(c, n, nullptr, nullptr)) return rc;
  HIPCHECK(hipSetDevice(c->cfg.device));
  MatchFramesArgs a = match_frames_args(c, n, nullptr, nullptr);
  a.cross_check = cross_check != 0;
  bank_as_train(a, c->bank, slot);
  MatchPoseArgs g = match_pose_args(c, R, t, fx, fy, cx, cy, radius);
  g.lm = c->lm_xyzw;                                            // (null without a landmark reservation)
  return match_guided_launch(c, GUIDED_POSE, a, MatchGuidedArgs{}, n, max_dist, ratio, match, dist, nullptr, &g);
}

// ---- landmarks for a new key frame from its PnP pose (include/fpc.h; kernel in landmarks.h) -----------------------------------
// One launch per call: the kernel reads every row straight from its source, so there is no pair list, no workspace and no
// reservation behind these calls.
int fpc_default_landmark_params(fpc_landmark_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->reproj_threshold = 3.0f;
  p->min_parallax_deg = 1.0f;
  return FPC_OK;
}

static bool landmark_params_ok(const fpc_landmark_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         threshold_ok(p->reproj_threshold) && p->min_parallax_deg >= 0.f && p->min_parallax_deg < 90.f;   // (a NaN fails)
}

// what the three calls share behind their source's own checks: the arguments every source has, then the launch; S rows of
// xyz / kind per frame
extern "C++" template <class Source>    // (this block is extern "C")
static int landmarks_launch(fpc_ctx* c, int n, const Source& src, const float* R, const float* t, const fpc_landmark_params* p,
                            float* xyz, uint8_t* kind, int32_t* counts, int S) {
  if (!R || !t || !xyz || !kind || !landmark_params_ok(p)) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  LmArgs a{};
  a.q_fx = p->q_fx; a.q_fy = p->q_fy; a.q_cx = p->q_cx; a.q_cy = p->q_cy;
  a.t_fx = p->t_fx; a.t_fy = p->t_fy; a.t_cx = p->t_cx; a.t_cy = p->t_cy;
  a.thr = p->reproj_threshold;
  const double s = std::sin((double)p->min_parallax_deg * (3.14159265358979323846 / 180.0));
  a.parallax = p->min_parallax_deg > 0.f ? s * s : POSE_PARALLEL;
  hipLaunchKernelGGL(landmarks_kernel<Source>, dim3(n), dim3(256), 0, c->stream, src, a, R, t, xyz, kind, counts, S);
  return launched();
}

int fpc_landmarks_pairs(fpc_ctx* c, int n, const float* q_xy, const float* t_xy, const float* t_xyz, const uint8_t* t_valid,
                        const int32_t* npairs, int stride, const float* R, const float* t, const fpc_landmark_params* p,
                        float* xyz, uint8_t* kind, int32_t* counts) {
  if (!c || !q_xy || !t_xy || !npairs || !explicit_ok(c, n, stride)) return FPC_E_INVALID;
  LmExplicit src{};
  src.q_xy = q_xy; src.t_xy = t_xy; src.t_xyz = t_xyz; src.t_valid = t_valid; src.npairs = npairs; src.stride = stride;
  return landmarks_launch(c, n, src, R, t, p, xyz, kind, counts, stride);
}

int fpc_landmarks_frames(fpc_ctx* c, int n, const int32_t* key_xy, const int32_t* nkey, const float* key_xyz,
                         const uint8_t* key_valid, const int32_t* match, const float* R, const float* t,
                         const fpc_landmark_params* p, float* xyz, uint8_t* kind, int32_t* counts) {
  if (!c || !key_xy || !nkey || !match || !frames_ok(c, n)) return FPC_E_INVALID;
  LmKey src{};
  src.q = LmFrames{c->xy, c->count, match, c->cap};
  src.key_xy = key_xy; src.nkey = nkey; src.key_xyz = key_xyz; src.key_valid = key_valid;
  return landmarks_launch(c, n, src, R, t, p, xyz, kind, counts, c->cap);
}

int fpc_landmarks_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const float* R, const float* t,
                       const fpc_landmark_params* p, float* xyz, uint8_t* kind, int32_t* counts) {
  if (!c || !bank_ok(c, n, slot, match)) return FPC_E_INVALID;
  LmBank src{};
  src.q = LmFrames{c->xy, c->count, match, c->cap};
  src.slot = slot; src.bank_xy = c->bank.xy; src.bank_count = c->bank.count;
  src.bank_lm = c->lm_xyzw;                                      // (null without a landmark reservation: triangulation only)
  src.rows = c->bank.rows; src.slots = c->bank.slots;
  return landmarks_launch(c, n, src, R, t, p, xyz, kind, counts, c->cap);
}

// ---- two-view bundle adjustment of a pose call's R, t and points (include/fpc.h; kernel in refine_pose.h) --------------------
// The pose calls' pair sources with a NULL mask, their pair records and workspace: a refine call leaves the pair list its pose
// twin built, built again.
int fpc_default_refine_params(fpc_refine_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->reproj_threshold = 3.0f;
  p->min_parallax_deg = 1.0f;
  p->iterations = 8;
  p->lambda0 = 1e-3f;
  p->min_front = 8;
  return FPC_OK;
}

static bool refine_params_ok(const fpc_refine_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         threshold_ok(p->reproj_threshold) && p->min_parallax_deg >= 0.f && p->min_parallax_deg < 90.f &&   // (a NaN fails)
         p->iterations >= 1 && p->iterations <= 16 && std::isfinite(p->lambda0) && p->lambda0 > 0.f && p->min_front >= 1;
}

// what the three calls refuse before their pair source is looked at
static bool refine_ok(const fpc_ctx* c, const float* R_in, const float* t_in, const fpc_refine_params* p, const float* R,
                      const float* t, const int32_t* nfront, const float* xyz) {
  return c && R_in && t_in && R && t && nfront && xyz && refine_params_ok(p);
}

// the solver step behind the pair list (a: hf_args with the parameters' threshold, nothing of RANSAC's)
static int refine_launch(fpc_ctx* c, const HfArgs& a, const fpc_refine_params* p, const float* R_in, const float* t_in, float* R,
                         float* t, int32_t* nfront, float* xyz, uint8_t* front, float* stats, int ostride) {
  const double s = std::sin((double)p->min_parallax_deg * (3.14159265358979323846 / 180.0));
  const RefineArgs ra{p->q_fx, p->q_fy, p->q_cx, p->q_cy, p->t_fx, p->t_fy, p->t_cx, p->t_cy,
                      p->min_parallax_deg > 0.f ? s * s : POSE_PARALLEL, p->iterations, p->lambda0, p->min_front};
  hipLaunchKernelGGL(refine_pose_kernel, dim3(a.n), dim3(256), 0, c->stream, a, ra, R_in, t_in, R, t, nfront, xyz, front, stats,
                     ostride);
  return launched();
}

int fpc_refine_pose(fpc_ctx* c, int n, const float* src_xy, const float* dst_xy, const int32_t* npairs, int stride,
                    const float* R_in, const float* t_in, const fpc_refine_params* p, float* R, float* t, int32_t* nfront,
                    float* xyz, uint8_t* front, float* stats) {
  if (!refine_ok(c, R_in, t_in, p, R, t, nfront, xyz)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_explicit(c, a, src_xy, dst_xy, npairs, stride, nullptr)) return rc;
  return refine_launch(c, a, p, R_in, t_in, R, t, nfront, xyz, front, stats, stride);
}

int fpc_refine_pose_frames(fpc_ctx* c, int n, int pairing, const int32_t* key_xy, const int32_t* nkey, const int32_t* match,
                           const float* R_in, const float* t_in, const fpc_refine_params* p, float* R, float* t,
                           int32_t* nfront, float* xyz, uint8_t* front, float* stats) {
  if (!refine_ok(c, R_in, t_in, p, R, t, nfront, xyz)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_frames(c, a, pairing, key_xy, nkey, match, nullptr)) return rc;
  return refine_launch(c, a, p, R_in, t_in, R, t, nfront, xyz, front, stats, c->cap);
}

int fpc_refine_pose_bank(fpc_ctx* c, int n, const int32_t* slot, const int32_t* match, const float* R_in, const float* t_in,
                         const fpc_refine_params* p, float* R, float* t, int32_t* nfront, float* xyz, uint8_t* front,
                         float* stats) {
  if (!refine_ok(c, R_in, t_in, p, R, t, nfront, xyz)) return FPC_E_INVALID;
  const HfArgs a = hf_args(c, n, p->reproj_threshold);
  if (int rc = pairs_bank(c, a, n, slot, match, nullptr)) return rc;
  return refine_launch(c, a, p, R_in, t_in, R, t, nfront, xyz, front, stats, c->cap);
}

// ---- local bundle adjustment of a key frame's landmarks over up to 16 frames (include/fpc.h; kernels in refine_window.h) -----
int fpc_default_window_params(fpc_window_params* p) {
  if (!p) return FPC_E_INVALID;
  p->q_fx = p->q_fy = p->t_fx = p->t_fy = 500.0f;
  p->q_cx = p->t_cx = 320.0f;
  p->q_cy = p->t_cy = 240.0f;
  p->reproj_threshold = 3.0f;
  p->iterations = 8;
  p->lambda0 = 1e-3f;
  p->min_obs = 6;
  return FPC_OK;
}

// The only call of the section that allocates or synchronises: an allocation of its own (nothing is carved: the plan hash,
// the packed size and the bank's bytes are what they were).
int fpc_window_reserve(fpc_ctx* c, size_t* bytes) {
  if (!c || c->window_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t cap = c->cap, chunks = (cap + RW_CHUNK - 1) / RW_CHUNK;
  Carver cv(c);
  RwArgs& w = c->rw;
  cv.into(&w.st, 1); cv.into(&w.tab, RW_FRAMES * cap); cv.into(&w.pix, RW_FRAMES * cap); cv.into(&w.kpix, cap);
  cv.into(&w.lmk, cap); cv.into(&w.xd, cap * 3); cv.into(&w.xnew, cap * 3); cv.into(&w.part, chunks * RW_PART);
  cv.into(&w.cpart, chunks); cv.into(&w.bad, chunks);
  if (int rc = c->window_slab.allocate(c->stream, cv)) return rc;
  if (bytes) *bytes = c->window_slab.bytes;
  return FPC_OK;
}

static bool window_params_ok(const fpc_window_params* p) {
  return p && camera_ok(p->q_fx, p->q_fy, p->q_cx, p->q_cy) && camera_ok(p->t_fx, p->t_fy, p->t_cx, p->t_cy) &&
         threshold_ok(p->reproj_threshold) && p->iterations >= 1 && p->iterations <= 16 && std::isfinite(p->lambda0) &&
         p->lambda0 > 0.f && p->min_obs >= 3;                    // (a NaN fails its comparison)
}

// what the three calls share behind their source's own checks: the arguments every source has, then the launches -- the
// membership passes, C of the start, `iterations` times the attempt's five kernels (no-ops once the call has stopped on the
// device), the result.  S rows of obs per frame.
extern "C++" template <class Source>    // (this block is extern "C")
static int window_launch(fpc_ctx* c, int n, const Source& src, const float* R_in, const float* t_in, const fpc_window_params* p,
                         float* R, float* t, int32_t* nobs, float* xyz, uint8_t* kind, uint8_t* obs, float* stats, int S) {
  if (!c->window_slab || n > FPC_WINDOW_MAX_FRAMES || !R_in || !t_in || !R || !t || !nobs || !xyz || !kind || !window_params_ok(p))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  RwArgs a = c->rw;
  a.q_fx = p->q_fx; a.q_fy = p->q_fy; a.q_cx = p->q_cx; a.q_cy = p->q_cy;
  a.t_fx = p->t_fx; a.t_fy = p->t_fy; a.t_cx = p->t_cx; a.t_cy = p->t_cy;
  a.thr = p->reproj_threshold; a.iterations = p->iterations; a.lambda0 = p->lambda0; a.min_obs = p->min_obs;
  a.n = n; a.cap = c->cap; a.S = S; a.xyz = xyz;
  const int rows = (c->cap + 255) / 256, chunks = (c->cap + RW_CHUNK - 1) / RW_CHUNK;
  hipStream_t st = c->stream;
  HIPCHECK(hipMemsetAsync(a.tab, 0x7f, sizeof(int32_t) * RW_FRAMES * c->cap, st));
  HIPCHECK(hipMemsetAsync(nobs, 0, sizeof(int32_t) * n, st));
  if (obs) HIPCHECK(hipMemsetAsync(obs, 0, (size_t)n * S, st));
  hipLaunchKernelGGL(rw_init_kernel<Source>, dim3(rows), dim3(256), 0, st, src, a, R_in, t_in);
  hipLaunchKernelGGL(rw_members_kernel<Source>, dim3((S + 255) / 256, n), dim3(256), 0, st, src, a);
  hipLaunchKernelGGL(rw_resolve_kernel<Source>, dim3(rows, n), dim3(256), 0, st, src, a);
  hipLaunchKernelGGL(rw_finish_kernel, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(rw_cost_kernel, dim3(chunks), dim3(RW_CHUNK), 0, st, a, 0);
  hipLaunchKernelGGL(rw_decide_kernel, dim3(1), dim3(256), 0, st, a, 1);
  for (int it = 0; it < p->iterations; ++it) {
    hipLaunchKernelGGL(rw_build_kernel, dim3(chunks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rw_solve_kernel, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rw_step_kernel, dim3(chunks), dim3(RW_CHUNK), 0, st, a);
    hipLaunchKernelGGL(rw_cost_kernel, dim3(chunks), dim3(RW_CHUNK), 0, st, a, 1);
    hipLaunchKernelGGL(rw_decide_kernel, dim3(1), dim3(256), 0, st, a, 0);
  }
  hipLaunchKernelGGL(rw_final_kernel, dim3(rows), dim3(256), 0, st, a, R, t, nobs, kind, obs, stats);
  return launched();
}

int fpc_refine_window(fpc_ctx* c, int n, const float* xy, const int32_t* idx, const int32_t* nobs_in, int stride,
                      const float* key_xy, const float* key_xyz, const uint8_t* key_valid, const int32_t* nkey,
                      const float* R_in, const float* t_in, const fpc_window_params* p, float* R, float* t, int32_t* nobs,
                      float* xyz, uint8_t* kind, uint8_t* obs, float* stats) {
  if (!c || !xy || !idx || !nobs_in || !key_xy || !key_xyz || !nkey || !explicit_ok(c, n, stride)) return FPC_E_INVALID;
  const RwExplicit src{xy, idx, nobs_in, stride, key_xy, key_xyz, key_valid, nkey, c->cap};
  return window_launch(c, n, src, R_in, t_in, p, R, t, nobs, xyz, kind, obs, stats, stride);
}

int fpc_refine_window_frames(fpc_ctx* c, int n, const int32_t* key_xy, const int32_t* nkey, const float* key_xyz,
                             const uint8_t* key_valid, const int32_t* match, const float* R_in, const float* t_in,
                             const fpc_window_params* p, float* R, float* t, int32_t* nobs, float* xyz, uint8_t* kind,
                             uint8_t* obs, float* stats) {
  if (!c || !key_xy || !nkey || !key_xyz || !match || !frames_ok(c, n)) return FPC_E_INVALID;
  const RwKey src{RwFrames{c->xy, c->count, match, c->cap}, key_xy, key_xyz, key_valid, nkey};
  return window_launch(c, n, src, R_in, t_in, p, R, t, nobs, xyz, kind, obs, stats, c->cap);
}

int fpc_refine_window_bank(fpc_ctx* c, int n, const int32_t* key_slot, const int32_t* slot, const int32_t* match,
                           const float* R_in, const float* t_in, const fpc_window_params* p, float* R, float* t, int32_t* nobs,
                           float* xyz, uint8_t* kind, uint8_t* obs, float* stats) {
  if (!c || !c->bank_slab || !key_slot || !match || !frames_ok(c, n)) return FPC_E_INVALID;
  // (without landmark storage bank_lm is null: the key has no rows, and the call fails on the device)
  const RwBank src{RwFrames{c->xy, c->count, match, c->cap}, key_slot, slot, c->bank.xy, c->bank.count, c->lm_xyzw, c->bank.rows,
                   c->bank.slots};
  return window_launch(c, n, src, R_in, t_in, p, R, t, nobs, xyz, kind, obs, stats, c->cap);
}

// ---- pose graph over the bank's slots (include/fpc.h; kernels in pose_graph.h) ---------------------------------------------------
int fpc_default_graph_params(fpc_graph_params* p) {
  if (!p) return FPC_E_INVALID;
  p->iterations = 16;
  p->lambda0 = 1e-3f;
  p->cg_iterations = 256;
  p->cg_tol = 1e-8f;
  p->trans_unit = 1.0f;
  return FPC_OK;
}

// The only call of the section that allocates or synchronises: an allocation of its own (nothing is carved: the plan hash,
// the packed size and the bank's bytes are what they were).  Zeroed: every node unset, no edge.
int fpc_graph_reserve(fpc_ctx* c, int nodes, int edges, size_t* bytes) {
  if (!c || c->graph_slab || nodes < 1 || nodes > FPC_BANK_MAX_SLOTS || edges < 1 || edges > FPC_GRAPH_MAX_EDGES)
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const size_t N = nodes, E = edges, chunks = (E + PG_CHUNK - 1) / PG_CHUNK;
  Carver cv(c);
  PgArgs& g = c->pg;
  cv.into(&g.ns, N); cv.into(&g.nR, N * 9); cv.into(&g.nt, N * 3);
  cv.into(&g.efrom, E); cv.into(&g.eto, E); cv.into(&g.es, E); cv.into(&g.eR, E * 9); cv.into(&g.et, E * 3); cv.into(&g.ew, E);
  cv.into(&g.count, 2); cv.into(&g.st, 1);
  cv.into(&g.cs, N); cv.into(&g.cR, N * 9); cv.into(&g.ct, N * 3);
  cv.into(&g.deg, N + 1); cv.into(&g.adj, 2 * E); cv.into(&g.member, N); cv.into(&g.bad, N);
  cv.into(&g.lin, E * PG_LIN);
  cv.into(&g.g, (size_t)7 * PG_MAX_NODES); cv.into(&g.dH, (size_t)7 * PG_MAX_NODES); cv.into(&g.delta, (size_t)7 * PG_MAX_NODES);
  cv.into(&g.Minv, (size_t)49 * PG_MAX_NODES); cv.into(&g.cpart, chunks); cv.into(&g.eq, E * 8);
  if (int rc = c->graph_slab.allocate(c->stream, cv)) return rc;
  g.nodes = nodes; g.edges = edges;
  if (bytes) *bytes = c->graph_slab.bytes;
  return FPC_OK;
}

int fpc_graph_get(fpc_ctx* c, fpc_graph_view* v) {
  if (!c || !v || !c->graph_slab) return FPC_E_INVALID;
  const PgArgs& g = c->pg;
  v->nodes = g.nodes; v->edges = g.edges;
  v->node_s = g.ns; v->node_R = g.nR; v->node_t = g.nt;
  v->edge_from = g.efrom; v->edge_to = g.eto; v->edge_s = g.es; v->edge_R = g.eR; v->edge_t = g.et; v->edge_w = g.ew;
  v->count = g.count;
  v->bytes = c->graph_slab.bytes;
  return FPC_OK;
}

int fpc_graph_clear(fpc_ctx* c) {
  if (!c || !c->graph_slab) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const PgArgs& g = c->pg;
  HIPCHECK(hipMemsetAsync(g.ns, 0, sizeof(float) * g.nodes, c->stream));
  HIPCHECK(hipMemsetAsync(g.nR, 0, sizeof(float) * g.nodes * 9, c->stream));
  HIPCHECK(hipMemsetAsync(g.nt, 0, sizeof(float) * g.nodes * 3, c->stream));
  HIPCHECK(hipMemsetAsync(g.count, 0, sizeof(int32_t) * 2, c->stream));
  return FPC_OK;
}

int fpc_graph_set_nodes(fpc_ctx* c, int first, int count, const float* s, const float* R, const float* t) {
  if (!c || !c->graph_slab || !R || !t || first < 0 || count < 1 || first > c->pg.nodes - count) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(pg_set_nodes_kernel, dim3((count + 255) / 256), dim3(256), 0, c->stream, c->pg, first, count, s, R, t);
  return launched();
}

int fpc_graph_add_edges(fpc_ctx* c, int n, const int32_t* from, const int32_t* to, const float* s, const float* R, const float* t,
                        const int32_t* ninliers, int min_inliers, unsigned flags) {
  if (!c || !c->graph_slab || n < 1 || n > FPC_GRAPH_MAX_EDGES || !from || !to || !R || !t || (flags & ~FPC_GRAPH_INIT_TO))
    return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(pg_add_edges_kernel, dim3(1), dim3(256), 0, c->stream, c->pg, n, from, to, s, R, t, ninliers, min_inliers,
                     (flags & FPC_GRAPH_INIT_TO) ? 1 : 0);
  return launched();
}

static bool graph_params_ok(const fpc_graph_params* p) {
  return p && p->iterations >= 1 && p->iterations <= 16 && std::isfinite(p->lambda0) && p->lambda0 > 0.f &&
         p->cg_iterations >= 1 && p->cg_iterations <= 1024 && std::isfinite(p->cg_tol) && p->cg_tol >= 0.f &&
         std::isfinite(p->trans_unit) && p->trans_unit > 0.f;    // (a NaN fails its comparison)
}

// The launches: the problem (degrees, begin, adjacency), C of the start, `iterations` times the attempt's kernels (no-ops
// once the call has stopped on the device).
int fpc_graph_optimise(fpc_ctx* c, const int32_t* fixed, const fpc_graph_params* p, float* stats) {
  if (!c || !c->graph_slab || !fixed || !stats || !graph_params_ok(p)) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  PgArgs a = c->pg;
  a.iterations = p->iterations; a.cg_iterations = p->cg_iterations;
  a.lambda0 = (double)p->lambda0; a.tol2 = (double)p->cg_tol * (double)p->cg_tol; a.iu = 1.0 / (double)p->trans_unit;
  const int nchunks = (a.nodes + PG_CHUNK - 1) / PG_CHUNK, echunks = (a.edges + PG_CHUNK - 1) / PG_CHUNK;
  int wg = 64;
  while (wg < a.nodes) wg *= 2;                                  // the solve's workgroup: the power of two >= nodes
  hipStream_t st = c->stream;
  hipLaunchKernelGGL(pg_degree_kernel, dim3(nchunks), dim3(PG_CHUNK), 0, st, a);
  hipLaunchKernelGGL(pg_begin_kernel, dim3(1), dim3(1024), 0, st, a, fixed, stats);
  hipLaunchKernelGGL(pg_fill_kernel, dim3(nchunks), dim3(PG_CHUNK), 0, st, a);
  hipLaunchKernelGGL(pg_edges_kernel<false>, dim3(echunks), dim3(PG_CHUNK), 0, st, a);
  hipLaunchKernelGGL(pg_decide_kernel, dim3(1), dim3(1024), 0, st, a, 1, stats);
  for (int it = 0; it < p->iterations; ++it) {
    if (it) hipLaunchKernelGGL(pg_edges_kernel<false>, dim3(echunks), dim3(PG_CHUNK), 0, st, a);
    hipLaunchKernelGGL(pg_blocks_kernel, dim3(nchunks), dim3(PG_CHUNK), 0, st, a);
    hipLaunchKernelGGL(pg_solve_kernel, dim3(1), dim3(wg), 0, st, a);
    hipLaunchKernelGGL(pg_retract_kernel, dim3(nchunks), dim3(PG_CHUNK), 0, st, a);
    hipLaunchKernelGGL(pg_edges_kernel<true>, dim3(echunks), dim3(PG_CHUNK), 0, st, a);
    hipLaunchKernelGGL(pg_decide_kernel, dim3(1), dim3(1024), 0, st, a, 0, stats);
  }
  return launched();
}

int fpc_graph_apply_scale(fpc_ctx* c) {
  if (!c || !c->graph_slab || !c->bank_slab || !c->lm_slab || c->pg.nodes != c->bank.slots) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  const PgArgs& a = c->pg;
  hipStream_t st = c->stream;
  hipLaunchKernelGGL(pg_scale_edges_kernel, dim3((a.edges + 255) / 256), dim3(256), 0, st, a);
  hipLaunchKernelGGL(pg_scale_points_kernel, dim3((c->bank.rows + 255) / 256, c->bank.slots), dim3(256), 0, st, a, c->lm_xyzw,
                     c->bank.count, c->bank.rows);
  hipLaunchKernelGGL(pg_scale_nodes_kernel, dim3((a.nodes + 255) / 256), dim3(256), 0, st, a);
  return launched();
}

int fpc_results(fpc_ctx* c, fpc_device_results* out) {
  if (!c || !out) return FPC_E_INVALID;
  out->count = c->count;
  out->n_candidates = c->ncand;
  out->xy = c->xy;
  out->conf = c->conf;
  out->desc = c->cfg.descriptor_enabled ? c->desc_out : nullptr;
  out->capacity = c->cap;
  out->desc_dim = c->D;
  return FPC_OK;
}

int fpc_get_counts(fpc_ctx* c, int n, int32_t* count, int32_t* ncand) {
  if (!c || n < 1 || n > c->B) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipStreamSynchronize(c->stream));
  int32_t st[2] = {0, 0};
  HIPCHECK(hipMemcpy(st, c->status, sizeof(st), hipMemcpyDeviceToHost));
  if (st[0]) return FPC_E_NOT_CONVERGED;
  if (st[1]) return FPC_E_RANGE;
  if (count) HIPCHECK(hipMemcpy(count, c->count, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (ncand) HIPCHECK(hipMemcpy(ncand, c->ncand, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  // a frame with a NaN / Inf pixel (FPC_F32's stem looks at every pixel it stages): the counts above are delivered, the
  // call is flagged -- include/fpc.h, FPC_E_NONFINITE
  std::vector<uint32_t> rw((size_t)n * FPC_RANGE_WORDS);
  HIPCHECK(hipMemcpy(rw.data(), c->range, rw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (int b = 0; b < n; ++b)
    if (rw[(size_t)b * FPC_RANGE_WORDS + RANGE_BAD_INPUT]) {
      g_hip_err = "frame " + std::to_string(b) + " of the last call holds a NaN or Inf pixel";
      return FPC_E_NONFINITE;
    }
  return FPC_OK;
}

int fpc_output_range(fpc_ctx* c, int n, float* max_logit, float* max_desc, int32_t* nonfinite_input) {
  if (!c || n < 1 || n > c->B) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipStreamSynchronize(c->stream));
  std::vector<uint32_t> rw((size_t)n * FPC_RANGE_WORDS);
  HIPCHECK(hipMemcpy(rw.data(), c->range, rw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<float> rm((size_t)n * c->Hc);
  if (max_logit) HIPCHECK(hipMemcpy(rm.data(), c->rowmax, rm.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int b = 0; b < n; ++b) {
    const uint32_t* w = rw.data() + (size_t)b * FPC_RANGE_WORDS;
    float f;
    if (max_logit) {
      f = 0.f;
      for (int i = 0; i < c->Hc; ++i) f = std::max(f, rm[(size_t)b * c->Hc + i]);
      max_logit[b] = f;
    }
    if (max_desc) { memcpy(&f, w + RANGE_MAX_DESC, 4); max_desc[b] = f; }
    if (nonfinite_input) nonfinite_input[b] = (int32_t)w[RANGE_BAD_INPUT];
  }
  return FPC_OK;
}

int fpc_get_keypoints(fpc_ctx* c, int frame, int cap, int32_t* xy, float* conf, float* desc) {
  if (!c || frame < 0 || frame >= c->B || cap < 0) return FPC_E_INVALID;
  HIPCHECK(hipSetDevice(c->cfg.device));
  HIPCHECK(hipStreamSynchronize(c->stream));
  int32_t k = 0;
  HIPCHECK(hipMemcpy(&k, c->count + frame, sizeof(k), hipMemcpyDeviceToHost));
  if (k > cap || k > c->cap) return FPC_E_CAPACITY;
  if (k == 0) return 0;
  if (xy) HIPCHECK(hipMemcpy(xy, c->xy + (size_t)frame * c->cap * 2, sizeof(int32_t) * 2 * k, hipMemcpyDeviceToHost));
  if (conf) HIPCHECK(hipMemcpy(conf, c->conf + (size_t)frame * c->cap, sizeof(float) * k, hipMemcpyDeviceToHost));
  if (desc) {
    if (!c->cfg.descriptor_enabled) return FPC_E_INVALID;
    HIPCHECK(hipMemcpy(desc, c->desc_out + (size_t)frame * c->cap * c->D, sizeof(float) * c->D * k, hipMemcpyDeviceToHost));
  }
  return k;
}

int fpc_set_timing(fpc_ctx* c, int enable) {
  if (!c) return FPC_E_INVALID;
  c->timing_every = enable > 0 ? enable : 0;
  c->timing_calls = 0;
  c->timing = enable != 0;
  c->timings.clear();   // records accumulate over calls from here on
  c->events_used = 0;
  return FPC_OK;
}

int fpc_get_timings(fpc_ctx* c, int cap, const char** names, const char** kernels, float* ms, double* flops,
                    double* mfma_flops, double* bytes) {
  if (!c) return FPC_E_INVALID;
  const int n = (int)c->timings.size();
  for (int i = 0; i < n && i < cap; ++i) {
    const Timing& t = c->timings[i];
    float v = 0.f;
    if (hipEventElapsedTime(&v, t.start, t.stop) != hipSuccess) v = -1.f;
    const Op* op = t.op >= 0 ? &c->ops[t.op] : nullptr;
    if (names) names[i] = op ? op->name.c_str() : "?";
    if (kernels) {
      const char* k = "?";
      if (op) switch (op->type) {
          case OP_STEM: k = launch_stem(c, *op, t.op, nullptr, nullptr); break;   // (no Sub: the name alone)
          case OP_POOL: k = "maxpool_kernel"; break;
          case OP_CONV: k = op->lean ? lean_kind(op->kind)->symbol : g_kinds[op->kind].symbol; break;
          case OP_BLOCK: k = g_bkinds[op->bkind].symbol; break;
          case OP_WBLOCK: k = g_wkinds[t.wkind >= 0 ? t.wkind : op->wkind].symbol; break;
          case OP_BF16: k = g_fkinds[op->fkind].symbol; break;
          case OP_SOFTMAX: k = "softmax_d2s_kernel"; break;
          case OP_NMS: k = c->opt.nms_one_workgroup ? "nms_rounds_kernel+nms_sort_kernel" : "nms_rounds_kernel+nms_finish_kernel+nms_chunk_sort_kernel+nms_merge_kernel"; break;
          case OP_DESC: k = "descriptor16_kernel"; break;
          case OP_VCONV0: k = "vgg_conv0_kernel"; break;
          case OP_POOL2: k = "maxpool2_kernel"; break;
          case OP_L2NORM: k = "l2norm256_kernel"; break;
        }
      kernels[i] = k;
    }
    if (ms) ms[i] = v;
    if (flops) flops[i] = op ? op->flops_per_frame * t.frames : 0.0;
    if (mfma_flops) mfma_flops[i] = !op ? 0.0 : t.mfma_flops >= 0 ? t.mfma_flops : op->mfma_flops_per_frame * t.frames;
    if (bytes) bytes[i] = op ? op->bytes_per_frame * t.frames : 0.0;
  }
  return n;
}

}  // extern "C"
