/*
 * fpc.h -- C-ABI of the MI355X-native SuperPoint inference path (libfpc.so).
 *
 * The reference (Kolkir/feature-point-cnn) has no plugin / FFI interface for this
 * path: its boundary is a pair of plain classes,
 *     C++    superpoint::SuperPoint            cpp/src/superpoint.h:12-36
 *     Python InferenceWrapper / SuperPoint     python/src/inferencewrapper.py:12-46,
 *                                              python/src/superpoint.py:64-115
 * Each entry point below names the reference code it stands in for.  Plain
 * pointers and sizes only; no torch / OpenCV types cross this boundary.  Every
 * function returns FPC_OK (0) or a negative FPC_E_* code -- nothing exits or
 * throws across the ABI (the reference exit()s: cpp/src/superpoint.cc:56-59,
 * python/src/saveutils.py:11-14).
 *
 * Threading: one fpc_ctx per GPU; calls on one ctx are serialised by the caller
 * (the reference object is not re-entrant either: cpp/src/superpoint.h:31-35);
 * distinct contexts are independent.
 *
 * There is no CPU fallback: without a HIP device fpc_create fails with
 * FPC_E_NO_DEVICE.
 */
#ifndef FPC_H
#define FPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPC_ABI_VERSION 4
/* Revision of the packed-weight FRAGMENT LAYOUTS (what the packing routines of this build write at the offsets the launch
 * plan names).  It is part of the blob's tag and of fpc_plan_hash: bump it whenever a packing routine changes the order
 * of values inside a layer's fragments -- offsets and sizes, which the plan hash covers anyway, do not change then, and
 * a blob of the older build would otherwise be accepted and multiplied with the wrong weights.
 *   1: rounds 1-2.   2: round 3 (fp32 stem fragments in the column / row tap-pair K order, stem_pair).
 *   3: round 4.  (ABI 4, round 5: fpc_stream_report added, fpc_set_stream's contract narrowed.)
 *   4: round 5 (fp32 stem fragments carry the folded-BN bias as a K step where stem_pool2_kernel runs; FPC_BF16's
 *      ConvTranspose fragments in convt_bf16_kernel's nine-taps-per-step order). */
#define FPC_PACK_LAYOUT_REVISION 4

enum {
  FPC_OK = 0,
  FPC_E_INVALID = -1,     /* bad argument / unsupported geometry                  */
  FPC_E_NO_DEVICE = -2,   /* no usable HIP device                                 */
  FPC_E_HIP = -3,         /* a HIP runtime call failed (fpc_last_hip_error)       */
  FPC_E_NO_WEIGHTS = -4,  /* forward/detect before any weights were loaded        */
  FPC_E_MISSING_KEY = -5, /* checkpoint entry missing or of the wrong shape       */
  FPC_E_CAPACITY = -6,    /* caller buffer too small (needed size is reported)    */
  FPC_E_NOT_CONVERGED = -7, /* NMS round limit hit (never seen)    */
  FPC_E_RANGE = -8,       /* FPC_F32_SPLIT_F16 only: a folded weight (at load) or an */
                          /* activation (reported by fpc_get_counts) left fp16's     */
                          /* range |x| <= 65504; use FPC_F32_SPLIT or FPC_F32        */
  FPC_E_NONFINITE = -9    /* fpc_get_counts: a frame of the call held a NaN or +-Inf */
                          /* pixel (see "Numerical contract" below)                  */
};

/* Numerical contract of FPC_F32 (the default), measured against a double-accumulating restatement of the reference on
 * checkpoints whose every activation was scaled x1 .. x100 (tests/test_gpu_round5.py):
 *  - the PRODUCTS of the path -- probability map, keypoint coordinates and confidences, unit-norm descriptors -- are
 *    within 1e-4 (measured <= 1.7e-5) / identical sets at every magnitude the reference itself survives: its softmax has
 *    no max-subtraction (python/src/superpoint.py:111-112), so logits above 88.7 overflow exp() there and here alike
 *    (NaN probabilities, no keypoint in such a cell);
 *  - the dense fp32 tensors fpc_forward returns (logits, descriptor map) carry fp32's RELATIVE error:
 *    |delta| <= 2.5e-6 * max|tensor| (measured 1.5e-6; the 3x3 layers run as Winograd F(4x4,3x3), whose F(2x2,3x3) and
 *    direct alternatives measure 1.0-1.7x smaller, i.e. the bound is fp32 accumulation over 12 layers, not the
 *    transform).  An ABSOLUTE 1e-4 therefore holds while max|tensor| <= 40 (13 ulp of fp32 at 64): fpc_output_range
 *    reports the magnitudes of the last call so that a caller who needs the absolute bar can check it;
 *  - frames must be finite.  FPC_F32's stem looks at every pixel it stages: a NaN or +-Inf pixel makes fpc_get_counts
 *    return FPC_E_NONFINITE for the call (after delivering the counts) and fpc_output_range name the frame.  The other
 *    frames of the batch are unaffected (frames are independent), and the call is memory-safe; the flagged frame's own
 *    results are UNDEFINED -- the reference propagates the NaN through the receptive field of the pixel (a region of
 *    NaN logits, no keypoints there), this library's ReLU (v_max_f32 returns the non-NaN operand) does not, and its
 *    Winograd tiles spread whatever survives further than a direct convolution would.  fpc_detect_u8* inputs are 8-bit
 *    and cannot be non-finite.  The other dtype modes do not check. */

enum { FPC_F32 = 0, FPC_BF16 = 1, FPC_F32_SPLIT = 2, FPC_F32_SPLIT_F16 = 3 };
enum { FPC_ARCH_RESNET = 0, FPC_ARCH_VGG = 1 };

/* Replaces SuperPointSettings (python/src/settings.py:2-8) / Settings
 * (cpp/src/settings.h:27-31) plus the geometry the reference takes from the frame. */
typedef struct fpc_config {
  int device;             /* HIP device ordinal                                    */
  int height, width;      /* frame size; multiples of 16 (8 if descriptor_enabled=0)*/
  int max_batch;          /* frames per fpc_detect / fpc_forward call              */
  int cell;               /* 8   settings.py:7   (only 8 is supported)             */
  int nms_dist;           /* 4   settings.py:4                                     */
  float conf_thresh;      /* 0.015 settings.py:5; finite and >= 0 (probabilities)  */
  int border_remove;      /* 4   settings.py:8                                     */
  int descriptor_enabled; /* 0 = MagicPoint, detector only (superpoint.py:103-109) */
  int max_keypoints;      /* per-frame output capacity; 0 = worst case for nms_dist; */
                          /* a smaller value keeps the most confident points        */
  int in_channels;        /* 0 or 3: frames [n,3,H,W] (superpoint.py:12); 1: gray frames   */
                          /* [n,1,H,W] -- what the reference feeds after replicating the   */
                          /* plane x3 (dataset_utils.py:19-20, cpp/src/camera.cc:17-18)    */
  int dtype;              /* FPC_F32 (0): fp32 activations and weights, the reference's    */
                          /* arithmetic; FPC_BF16 (1): bf16 activations / weights with     */
                          /* fp32 accumulation (BASELINE.json configs[4]); FPC_F32_SPLIT   */
                          /* (2): fp32 tensors, matrix products on the bf16 pipe with each */
                          /* operand split exactly into three bf16 terms (block_x3.h):     */
                          /* fp32-level accuracy, same 1e-4 parity bar as FPC_F32;         */
                          /* FPC_F32_SPLIT_F16 (3): the same with two fp16 terms per        */
                          /* operand and three MFMAs per product (faster; operands must lie */
                          /* in fp16's range, |x| <= 65504, or they saturate)               */
  int arch;               /* FPC_ARCH_RESNET (0): the Python network (superpoint.py), 128-D; */
                          /* FPC_ARCH_VGG (1): the C++ frontend's superpoint::SPModel        */
                          /* (cpp/src/model.cc, settings.h:19-25): gray input                */
                          /* (in_channels = 1), 256-D descriptors, fp32 or split mode        */
  /* Launch-plan knobs (zeros = the default plan).  The FPC_* environment variables of the
   * same names still override them, for A/B runs of an unmodified caller.  Variables with no field or flag here
   * (csrc/plan_options.h has the whole table): FPC_W36_CUS (CUs a persistent F(4x4,3x3) launch may take, 0 = all),
   * FPC_BF16_GRID (workgroups a persistent FPC_BF16 launch may take, 0 = blocks per CU x CUs), FPC_PERSIST_MIN,
   * FPC_NMS_G, FPC_MIN_SUB, FPC_STREAMS. */
  int num_streams;        /* sub-batches of one call on separate HIP streams; 0 = default (2; 3 in split modes)  */
  unsigned plan_flags;    /* FPC_PLAN_* bits                                                                   */
  int nms_round_launches; /* parallel NMS launches before the per-frame finish: 0 = default (2), -1 = none     */
  int min_sub_batch;      /* smallest sub-batch worth its own stream: 0 = default (8); calls below twice this   */
                          /* take the latency plan                                                             */
} fpc_config;

enum {
  FPC_PLAN_NO_FUSED_BLOCKS = 1 << 0,       /* conv1 / conv2 of a ResNetBlock as two launches            (FPC_FUSE=0)         */
  FPC_PLAN_NO_WINOGRAD = 1 << 1,           /* direct 3x3 convolutions everywhere                        (FPC_WINOGRAD=0)     */
  FPC_PLAN_NO_WINOGRAD_DETECTOR = 1 << 2,  /* ... in the detector's 65-channel blocks only              (FPC_WINOGRAD_DET=0) */
  FPC_PLAN_NO_WINOGRAD_LAYER_IN1 = 1 << 3, /* descriptor.layer_in.1 as the fused direct block           (FPC_WINOGRAD_IN1=0) */
  FPC_PLAN_NO_XCD_ORDER = 1 << 4,          /* plain tile order instead of the XCD-aware one             (FPC_XCD_ORDER=0)    */
  FPC_PLAN_NO_FUSED_STEM_POOL = 1 << 5,    /* stem convolution and max-pool as two launches             (FPC_FUSE_STEM=0)    */
  FPC_PLAN_SPLIT_HEADS = 1 << 6,           /* detector head + NMS on a side stream next to the descriptor head (FPC_SPLIT_HEADS=1): the
                                            * default, since round 4, of the Python network in FPC_F32 with two or more sub-batches */
  FPC_PLAN_NMS_IN_LINE = 1 << 7,           /* NMS on the sub-batch stream, not on a side stream         (FPC_NMS_ASIDE=0)    */
  FPC_PLAN_NO_PERSISTENT_GRID = 1 << 8,    /* one workgroup per tile in the Winograd kernels            (FPC_PERSIST_MIN=0)  */
  FPC_PLAN_LAYER1_TILE_8x16 = 1 << 9,      /* direct layer1 blocks on 8x16 instead of 16x16 tiles       (FPC_L1_T816=1)      */
  FPC_PLAN_WINOGRAD_GEN1 = 1 << 10,        /* round-1 Winograd kernel for the 64- / 128-channel layers  (FPC_WINOGRAD_GEN=1) */
  FPC_PLAN_NO_LATENCY_TILES = 1 << 11,     /* calls of a few frames keep the 8x16 tiles of the batch plan (FPC_LATENCY_TILES=0) */
  FPC_PLAN_NMS_ONE_WORKGROUP = 1 << 12,    /* survivors of a frame sorted by one workgroup, not in slices (FPC_NMS_CHUNKED=0)   */
  FPC_PLAN_NO_FUSED_SOFTMAX = 1 << 13,     /* FPC_BF16: exp-softmax as its own launch in fpc_detect too  (FPC_FUSE_SOFTMAX=0)   */
  FPC_PLAN_WINOGRAD_GEN2 = 1 << 14,        /* round-2 Winograd kernel, F(2x2,3x3), instead of F(4x4,3x3) (FPC_WINOGRAD_GEN=2)   */
  FPC_PLAN_HEADS_IN_LINE = 1 << 17,        /* ... and its opt-out: the two heads of a sub-batch back to back on its stream  (FPC_SPLIT_HEADS=0) */
  FPC_PLAN_DETECTOR_GEN1 = 1 << 16,        /* the detector's 65-channel blocks on round 1's kernel in batch calls too       (FPC_WINOGRAD_DET_GEN=1) */
  FPC_PLAN_W36_ONE_WAVE = 1 << 18,         /* the 64-channel F(4x4,3x3) layers on round 3's one-wave-per-SIMD kernel instead of round 5's two  (FPC_W36_PAIRED=0) */
  FPC_PLAN_STEM_ROUND3 = 1 << 20,          /* FPC_F32: round 3's stem_pool_kernel also where round 5's stem_pool2_kernel applies (conv map of whole 16x16 tiles) (FPC_STEM_LEAN=0) */
  FPC_PLAN_CONV_ROUND1 = 1 << 21,          /* FPC_F32: round 1's conv_mfma_kernel also where round 5's conv2_mfma_kernel applies (ConvTranspose, layer_in.1's 1x1) (FPC_CONV_LEAN=0) */
  FPC_PLAN_CONVT_PHASES = 1 << 19,         /* FPC_BF16: the ConvTranspose as four output-parity launches (rounds 2-4) instead of round 5's one  (FPC_CONVT_FUSED=0) */
  FPC_PLAN_TILES_ROUND5 = 1 << 22,         /* FPC_F32: round 5's tilings where round 6 picks the tile that issues fewer padded matrix rows (layer2.0 on 3x20 instead of 4x16); same blob, same plan hash, same results bit for bit  (FPC_TILES_ROUND6=0) */
  FPC_PLAN_GUARD_ZONES = 1 << 15           /* TEST FACILITY: 64 KiB of a canary pattern behind every buffer of the workspace and
                                              2 GiB behind the last one (the workspace grows by that much); fpc_check_guards
                                              counts the words a kernel has overwritten.  Not for production contexts.          */
};

/* One checkpoint entry: name and shape as in ckpt['model_state_dict']
 * (python/src/saveutils.py:57-62), data in host memory. */
typedef struct fpc_tensor {
  const char* name;
  const float* data;      /* float32, contiguous, PyTorch layout                   */
  int ndim;
  int64_t shape[4];
} fpc_tensor;

/* Device-resident results of the last fpc_detect call (zero-copy view). */
typedef struct fpc_device_results {
  const int32_t* count;       /* [n]            keypoints per frame (after border crop)    */
  const int32_t* n_candidates;/* [n]            pixels that passed conf_thresh             */
  const int32_t* xy;          /* [n][cap][2]    x, y                                       */
  const float* conf;          /* [n][cap]       descending (ties: row-major index ascending)*/
  const float* desc;          /* [n][cap][D]    unit L2 norm; NULL when descriptors are off */
  int capacity;               /* cap                                                       */
  int desc_dim;               /* D = 128 (256 for FPC_ARCH_VGG)                            */
} fpc_device_results;

typedef struct fpc_ctx fpc_ctx;

int fpc_abi_version(void);
/* "arch=gfx950;diag=0;ablations=none" for the product library: the code-object target, whether in-kernel stamps are
 * compiled in (the diagnostic build, never shipped), and that no experiment switch reached the build.  Static string. */
const char* fpc_build_flags(void);
const char* fpc_strerror(int code);
/* Text of the last HIP error seen by this thread (for FPC_E_HIP). */
const char* fpc_last_hip_error(void);

/* Fills the reference's defaults (settings.py:2-8), 480x640, max_batch 1. */
int fpc_default_config(fpc_config* cfg);

/* ~ SuperPoint::SuperPoint (cpp/src/superpoint.cc:9-66) / InferenceWrapper.__init__
 * (python/src/inferencewrapper.py:13-27) minus the file parsing: allocates the
 * device workspace for max_batch frames.  FPC_E_INVALID for a geometry the kernels cannot tile (height / width below
 * 16 or not a multiple of the network's stride, width above 3328, 2^30 pixels or more per frame) and for
 * max_batch * height * width >= 2^28 (the kernels address the tensors of a batch with 32-bit byte offsets, up to 16
 * bytes per frame pixel: 64 frames of 1280x960 are 2^26.2; larger jobs run as several calls or contexts).
 * FPC_ARCH_VGG keeps 256 bytes per frame pixel at full resolution: a plan that runs those layers on the generation-2
 * Winograd kernel in every call (FPC_PLAN_WINOGRAD_GEN2, or a frame of 2^23 pixels or more on the default plan) is
 * FPC_E_INVALID where max_batch * height * width * 256 exceeds 0xfffffff0 -- fourteen frames of 1280x960. */
int fpc_create(fpc_ctx** out, const fpc_config* cfg);
void fpc_destroy(fpc_ctx* ctx);

/* ~ load_checkpoint_for_inference (python/src/saveutils.py:6-18), strict: every
 * learnable entry of table W must be present with the right shape
 * (`num_batches_tracked` entries are ignored).  Folds BatchNorm (eval mode,
 * eps 1e-5) into the convolutions and packs MFMA fragments on the device.
 * With descriptor_enabled == 0 the `descriptor.*` entries may be absent. */
int fpc_load_weights(fpc_ctx* ctx, const fpc_tensor* tensors, int n);

/* Packed, folded weights as one blob -- what rank 0 broadcasts over RCCL/xGMI
 * instead of every rank parsing the checkpoint.  Layout is private to one build. */
size_t fpc_packed_size(const fpc_ctx* ctx);
void* fpc_packed_device_ptr(fpc_ctx* ctx);              /* in-place collective target */
int fpc_export_packed(fpc_ctx* ctx, void* host_dst, size_t cap);
int fpc_import_packed(fpc_ctx* ctx, const void* host_src, size_t n);
/* The same from DEVICE memory (the receive buffer of a broadcast, another ctx's fpc_packed_device_ptr): the tag is read
 * back and checked, the blob is copied device to device.  Synchronous. */
int fpc_import_packed_device(fpc_ctx* ctx, const void* dev_src, size_t n);
/* Declares the blob at fpc_packed_device_ptr valid (after a broadcast into it).  The blob starts with a 64-byte tag
 * (magic, ABI version, dtype, arch, launch-plan hash, size); fpc_import_packed and this call refuse a blob whose tag
 * does not match the context (FPC_E_INVALID; fpc_last_hip_error says which field). */
int fpc_mark_weights_loaded(fpc_ctx* ctx);
/* Hash of everything the blob layout depends on -- equal on two contexts iff they can exchange packed weights. */
uint64_t fpc_plan_hash(const fpc_ctx* ctx);
/* FPC_PACK_LAYOUT_REVISION of the library as built (a binding compares it with the header it was written against). */
int fpc_pack_layout_revision(void);

/* Which tiling a launch plan picks for a map -- the plan's own choice functions, answered without a device or a context
 * (round 6; FPC_PLAN_TILES_ROUND5 in plan_flags gives round 5's answer).  FPC_E_INVALID for an unknown `what`.
 *   what = 0: the 128-channel F(4x4,3x3) blocks.  Tile rows of ONE launch of `frames` frames of H x W walked as one
 *             stacked image on 16 x 16 tiles, or 0 where the launch walks frame by frame (as few tiles, or fewer).
 *   what = 1: a conv-only 64-channel launch of the paired F(4x4,3x3) kernel on an H x W map: its tile as
 *             100 x tile height + tile width in pixels (1616, 832, or 3208 = the 8 x 2 arrangement).
 *   what = 2: the stride-2 128-channel fused block (encoder.layer2.0) with an H x W OUTPUT: its tile likewise (320 or 416). */
int fpc_tile_choice(int what, int H, int W, int frames, unsigned plan_flags);

/* TEST FACILITY (contexts created with FPC_PLAN_GUARD_ZONES only; FPC_E_INVALID otherwise): waits for the device, then
 * counts the 32-bit words of the workspace's canary zones -- behind every activation / result buffer, and 2 GiB behind
 * the last one -- that no longer hold the pattern written at fpc_create.  0 = no kernel stored outside its tensors. */
int fpc_check_guards(fpc_ctx* ctx, long long* bad_words);

/* Frame-batch sharding over the GPUs of a node (the heaviest batch caller to shard is
 * python/src/preprocess_coco.py:64-74): the ONE exchange of the path.  The root rank has loaded the checkpoint
 * (fpc_load_weights); every rank of the communicator calls this with its own ctx, and receives the packed, BN-folded
 * blob by ncclBroadcast (RCCL over xGMI) straight into its device buffer -- no other rank parses the file.
 * nccl_comm is an ncclComm_t (passed as void* so that this header needs no rccl.h); librccl.so is resolved at run
 * time (FPC_E_HIP if absent).  Two collectives on the ctx stream: the 64-byte tag, then the blob; a root without
 * weights makes every rank return FPC_E_NO_WEIGHTS after the first; a rank whose ctx (dtype, arch, plan, build)
 * differs from the root's still completes both collectives, then returns FPC_E_INVALID.  Synchronous. */
int fpc_broadcast_weights(fpc_ctx* ctx, void* nccl_comm, int root);

/* Work is enqueued on this hipStream_t (default: a stream the ctx owns).  A stream handed in must stay valid until
 * fpc_destroy or the next fpc_set_stream.  Handing over the stream the ctx already runs on returns at once (cheap enough
 * to do before every call).  A NEW caller stream is looked at once: if it is idle and not being captured into a graph,
 * one ~40 us one-thread kernel is launched on it to learn which hardware queue it sits on (so that the ctx's sub-batch
 * streams can keep clear of that queue); a busy or capturing stream, the null stream, or FPC_QUEUE_PROBE=0: nothing is
 * launched and the ctx's other streams stay as they are.  Never synchronises the caller's stream. */
int fpc_set_stream(fpc_ctx* ctx, void* hip_stream);
void* fpc_get_stream(fpc_ctx* ctx);
/* A hipStream_t for the CALLER's uploads (hipMemcpyAsync of the next batch while this one computes): non-blocking, owned
 * by the ctx (destroyed with it), made at the first call.  It is chosen -- by the probe fpc_create uses for the ctx's own
 * streams -- so that it does not share a hardware queue with the ctx's main / sub-batch streams nor, where a queue is
 * left, with those of the device's other live ctxs: an upload on a stream that shares a queue with compute waits behind
 * every launch in front of it.  Order it against fpc_detect with events, as any two streams.  NULL on failure.
 * (The reference uploads on the default stream: python/src/superpoint.py:98-99 `.cuda()`.) */
void* fpc_upload_stream(fpc_ctx* ctx);
/* How the ctx's streams were placed on the GPU's hardware queues, and what that cost (csrc/queue_map.h).  The HIP runtime
 * maps streams onto GPU_MAX_HW_QUEUES (4) queues and two streams on one queue run their kernels in a row, so fpc_create
 * picks streams that sit on queues of their own.  queue[i] of stream slot[i] (0 = main, 1.. = sub-batch streams, 100.. =
 * side streams, 200 = upload stream): index of the hardware queue, -1 = a queue outside the map, -3 = not probed
 * (FPC_QUEUE_PROBE=0, a caller stream that was busy, or probing switched off after inconclusive rounds: `probing` 0).
 * process_* count every probe round of the process on this device; create_* what THIS ctx's fpc_create spent. */
typedef struct fpc_stream_report_t {
  int n_streams;
  int slot[16], queue[16];
  int probing;
  int hw_queues_found;
  int process_probe_rounds, process_probe_launches, process_inconclusive_rounds;
  float process_probe_ms;
  int create_probe_rounds;
  float create_placement_ms;
  int process_registered_streams;   /* streams of ALL live ctxs of the process in the registry (0 once every ctx is gone) */
} fpc_stream_report_t;
int fpc_stream_report(fpc_ctx* ctx, fpc_stream_report_t* out);
int fpc_sync(fpc_ctx* ctx);

/* ~ SuperPoint.forward (python/src/superpoint.py:91-115): frames [n,3,H,W] ([n,1,H,W] with
 * in_channels = 1) float32
 * on the device -> prob_map [n,H,W], desc [n,128,H/8,W/8], logits [n,65,H/8,W/8]
 * (device, NCHW like the reference; any output may be NULL).  Asynchronous. */
int fpc_forward(fpc_ctx* ctx, const float* frames_dev, int n, float* prob_map_dev,
                float* desc_dev, float* logits_dev);

/* The intermediate tensors the last fpc_forward / fpc_detect left in the workspace -- what a forward hook on the
 * reference's modules returns -- for per-layer parity tests (SURVEY.md 8c fixture F1).  name: "pool" (encoder.max_pool),
 * "layer1.0", "layer1.1", "layer2.0", "layer2.1" (encoder blocks), "det.0", "det.1" (= logits), "desc_in.0",
 * "desc_in.1", "up" (descriptor.relu after the transposed convolution + bn), "desc_out.0", "desc_out.1" (= the
 * descriptor map).  Frames frame0 .. frame0+n-1 as float32 NCHW into out_dev [n,C,h,w] (bf16 tensors of the FPC_BF16
 * mode are widened exactly); channels / height / width receive the tensor's shape (out_dev may be NULL to query it).
 * The fused kernels never write a block's inner tensor h nor the un-pooled stem output to memory: those have no name
 * here.  "det.1" exists only when the last call produced logits: fpc_forward always does; fpc_detect does except in
 * FPC_BF16 with the fused softmax epilogue (the default there; FPC_PLAN_NO_FUSED_SOFTMAX turns it off), where the
 * name returns FPC_E_INVALID instead of stale memory.
 * An FPC_ARCH_VGG context takes the names of superpoint::SPModel's modules instead: "conv0_a", "conv0_b", "pool0",
 * "conv1_a", "conv1_b", "pool1", "conv2_a", "conv2_b", "pool2", "conv3_a", "conv3_b" (the encoder: 64 channels on the
 * frame's size and at 1/2, 128 at 1/4 and 1/8; "poolN" is the 2 x 2 max-pool behind "convN_b"), "det_a" (256 channels),
 * "det_b" (= logits, 65), "desc_a" and "desc_b" (256; "desc_b" is the descriptor map as the forward leaves it, already
 * L2-normalised over its channels).  "desc_a" / "desc_b" return FPC_E_INVALID with the descriptor head disabled.
 * A name of the other network, or an unknown one, returns FPC_E_INVALID.  Asynchronous on the ctx stream. */
int fpc_read_activation(fpc_ctx* ctx, const char* name, int frame0, int n, float* out_dev, int* channels, int* height,
                        int* width);

/* ~ InferenceWrapper.run (inferencewrapper.py:29-46) / SuperPoint::ProcessFrame
 * (cpp/src/superpoint.cc:68-96) for n independent frames: forward, exp-softmax,
 * depth-to-space, threshold, greedy NMS, sort, border crop (netutils.py:78-100,
 * nms.py:4-53), descriptor sampling + L2 normalisation (netutils.py:103-121).
 * Asynchronous; results stay on the device until fetched. */
int fpc_detect(fpc_ctx* ctx, const float* frames_dev, int n);

/* The step in front of the path, on the device: 8-bit camera frames -> the float frames
 * fpc_detect takes, then fpc_detect.  Uploading u8 instead of fp32 RGB cuts the host-to-device bytes 4x
 * (12x for gray).  Conversion is `float32(u8) / 255.0f` (python/src/camera.py:31, dataset_utils.py:23,
 * preprocess_coco.py:25), written as planar [n,C,H,W] into a staging buffer the ctx allocates on first use.
 *   FPC_U8_GRAY         [n,H,W]    -> [n,1,H,W]  (ctx with in_channels = 1)
 *   FPC_U8_RGB_HWC      [n,H,W,3]  -> [n,3,H,W]  (ctx with in_channels = 3; inferencewrapper.py:70-81)
 *   FPC_U8_BGR_HWC      [n,H,W,3]  -> [n,3,H,W] with the channel swap of cv2.COLOR_BGR2RGB (inference.py:79)
 *   FPC_U8_BGR_HWC_GRAY [n,H,W,3]  -> [n,1,H,W]  cv::COLOR_BGR2GRAY on 8-bit data then convertTo(CV_32FC1,
 *                       1/255) (cpp/src/camera.cc:17-18): OpenCV's documented 14-bit fixed-point weights
 *                       (B 1868, G 9617, R 4899, +8192 >> 14) and a float multiply by (float)(1.0/255.0).
 *                       OpenCV is not available to this build: parity for THIS layout is unpinned.
 * Resizing (cv2.resize, inference.py:72-85) is not done here. */
enum { FPC_U8_GRAY = 0, FPC_U8_RGB_HWC = 1, FPC_U8_BGR_HWC = 2, FPC_U8_BGR_HWC_GRAY = 3 };
int fpc_detect_u8(fpc_ctx* ctx, const uint8_t* frames_dev, int n, int layout);
/* Camera frames of another size: make_query_image (python/src/inference.py:72-85) on the device, fused with the
 * conversion above -- ratio-preserving bilinear resize so that the frame covers the ctx's H x W (new size
 * int(src * max(H/src_h, W/src_w)) per axis), centre crop, /255, optional BGR -> RGB, HWC -> CHW -- then fpc_detect.
 * frames_dev [n,src_h,src_w,3] u8; layout FPC_U8_RGB_HWC or FPC_U8_BGR_HWC; a 3-channel ctx.  The bilinear rule
 * restates cv2.resize(INTER_LINEAR) on float32 data; pinned against torch's F.interpolate (same rule), not against
 * OpenCV (absent from this build). */
int fpc_detect_u8_resized(fpc_ctx* ctx, const uint8_t* frames_dev, int n, int src_h, int src_w, int layout);
/* The converted float frames of the last fpc_detect_u8 / fpc_detect_u8_resized call ([n,C,H,W], device) -- for tests. */
const float* fpc_u8_staging(fpc_ctx* ctx);

/* ~ homography_adaptation (python/src/homographies.py:250-324; the caller is
 * InferenceWrapper.run_with_homography_adaptation, inferencewrapper.py:48-68 <- preprocess_coco.py:64-74): the
 * probability maps of n frames aggregated over the un-warped view and `num` perspective views.  For view i the frames
 * are warped by homographies[i] (8 coefficients, the flattened 3x3 with h22 = 1, in the convention of
 * sample_homography :78-182), run through the network, masked, warped back with inverses[i] (NULL: computed here)
 * and accumulated with the validity counts; masks are eroded by an ellipse of radius erosion_radius
 * (config.valid_border_margin, 0 = off); aggregation 0 = 'sum' (count-normalised mean, the reference's default),
 * 1 = 'max'; pixels seen by fewer than num / 3 views become 0.  prob_out_dev [n,H,W] can be fed to fpc_get_points.
 * homographies / inverses are HOST arrays; frames and prob_out are device memory.  Asynchronous.
 * The warps restate torchvision's perspective() and the erosion OpenCV's erode(): both libraries are absent from this
 * build, see csrc/homography.h -- parity for this entry point is unpinned beyond torch's own grid_sample. */
int fpc_homography_adaptation(fpc_ctx* ctx, const float* frames_dev, int n, const float* homographies_host,
                              const float* inverses_host, int num, int erosion_radius, int aggregation,
                              float* prob_out_dev);

/* Runs only the post-processing of fpc_detect on a caller-provided probability map
 * [n,H,W] (device) -- get_points on its own (netutils.py:78-100). Descriptors are
 * sampled from desc_nchw_dev [n,128,H/8,W/8] when it is not NULL. */
int fpc_get_points(fpc_ctx* ctx, const float* prob_map_dev, const float* desc_nchw_dev, int n);

/* ~ get_descriptors(points, descriptors_map, img_h, img_w, settings) on its own (python/src/netutils.py:103-121):
 * bilinear grid_sample (align_corners=True, zero padding) of ONE descriptor map desc_nchw_dev [D,H/8,W/8] at k
 * caller-provided points, then division by the L2 norm (no epsilon: an all-zero sample gives NaN, as there).
 * xy_dev [k][2] float64 (x, y) in pixels of the ctx's H x W frame -- the first two rows of the reference's float64
 * `points`, transposed; the normalisation x / (W / 2) - 1 runs in double and is rounded to float once, as
 * `sample_points.float()` does.  out_dev [k][D] (the reference returns the transpose, [D][k]).  All device memory.
 * Asynchronous on the ctx stream.  Works with descriptor_enabled = 0 too (the map is the caller's). */
int fpc_sample_descriptors(fpc_ctx* ctx, const float* desc_nchw_dev, const double* xy_dev, int k, float* out_dev);

/* --- next row of the path: descriptor matching ----------------
 * ~ cv2.BFMatcher(cv2.NORM_L2, crossCheck=True).match(query, train) (python/src/inference.py:88-96):
 * for every query descriptor the nearest train descriptor in L2 (ties: lower index); with
 * cross_check != 0 only mutual nearest neighbours survive; with max_dist > 0 only matches closer
 * than max_dist.  q [nq][128], t [nt][128], match [nq] (train index or -1), dist [nq] (L2
 * distance to the nearest train descriptor; may be NULL) -- all device pointers; nq, nt <=
 * the ctx's keypoint capacity.  Asynchronous on the ctx stream.
 *
 * Non-finite descriptor rows.  Every matcher of this header evaluates d^2 = |q|^2 + |t|^2 - 2 q.t in fp32 (the bf16 bank:
 * on its rounded rows), and the rule is stated for that fp32 d^2: a pair whose d^2 is NaN or +inf -- a row that holds a
 * NaN or an Inf (an all-zero sample of fpc_sample_descriptors, caller memory), or finite rows whose fp32 norms overflow --
 * is never a row minimum, never a column minimum (it takes no part in the cross check), never a second best (it takes no
 * part in the ratio test) and never within a tolerance or below max_dist.  A query row with no train row at a finite
 * distance gets match -1 and dist +inf, as a query row with no train rows at all (nt = 0) does.  The other rows are
 * matched as if the non-finite rows were absent.  This is what cv2.BFMatcher and cpp/src/main.cc:18-29 do: a non-finite
 * distance is never a minimum and never below a tolerance. */
int fpc_match(fpc_ctx* ctx, const float* q_dev, int nq, const float* t_dev, int nt, int cross_check,
              float max_dist, int32_t* match_dev, float* dist_dev);
/* ~ SearchKeyFrameCorrespondence (cpp/src/main.cc:18-29,79-83): for every key-frame descriptor the
 * index of the FIRST current-frame descriptor (in the order given, i.e. descending confidence)
 * whose L2 distance is below `tolerance` (cpp/src/main.cc:54: 0.8), or -1.  A non-finite d^2 (fpc_match) is below no
 * tolerance: a non-finite key row gets -1, a non-finite current-frame row is nobody's first. */
int fpc_first_within(fpc_ctx* ctx, const float* key_dev, int nk, const float* cur_dev, int nc,
                     float tolerance, int32_t* first_dev);

/* --- the same two rules over a whole batch, straight from the device results -----------------------------------------
 * Frame f's query set is desc[f][0 .. count[f]) of fpc_results, from the last call that produced keypoints with
 * descriptors (fpc_detect, fpc_detect_u8*, fpc_get_points with a descriptor map); count[f] is read on the device.
 * FPC_E_INVALID when n exceeds that call's n, when it produced no descriptors, or with descriptor_enabled = 0.
 * Train set of frame f:  FPC_PAIR_KEY -- the key set;  FPC_PAIR_PREVIOUS -- frame f-1 of the same results for f >= 1;
 * frame 0 against the key set, or against nothing when key_dev is NULL (frame-to-frame tracking over a video batch).
 * Key set: key_dev [nkey][D] fp32 (D = desc_dim: 128, 256 for FPC_ARCH_VGG; 16-byte aligned), *nkey_dev an int32 in
 * device memory, read on the device and clamped to [0, cap] -- a frame kept from the previous call can be the key
 * without a host round trip.  nkey_dev is required whenever key_dev is given.
 *
 * fpc_match_frames: for every row i < count[f], exactly fpc_match(frame f, train(f), cross_check, max_dist); with
 * ratio > 0 also Lowe's test d1 < ratio * d2, d2 the distance to the second-nearest train row in (d^2, index) order
 * (fewer than two train rows: the test fails).  Enabled conditions are ANDed; dist = d1 as in fpc_match.  A row with
 * no train rows: match -1, dist +inf; rows count[f] <= i < cap: match -1 (dist +inf).  match_dev [n][cap],
 * dist_dev [n][cap] (may be NULL), cap = fpc_results().capacity.
 * FPC_E_INVALID also for a NULL ctx / output, a bad pairing, ratio outside [0, 1], max_dist < 0, a NULL key_dev with
 * FPC_PAIR_KEY.
 *
 * fpc_first_within_frames: for every key row j < nkey, fpc_first_within(key, frame f): the first row of frame f closer
 * than `tolerance`, or -1.  first_dev [n][cap]; rows j >= nkey get -1.  key_dev / nkey_dev required; tolerance >= 0.
 *
 * Both: asynchronous on the ctx stream (no host synchronisation, no device-to-host copy; may be enqueued right after
 * fpc_detect and before the next one), deterministic (bit-identical outputs on repeated calls).  Non-finite descriptor
 * rows, in a frame or in the key set: fpc_match's rule on the fp32 d^2 -- such a pair is no row minimum, no column minimum,
 * no second best and within no tolerance; a row with no train row at a finite distance: match -1, dist +inf. */
enum { FPC_PAIR_KEY = 0, FPC_PAIR_PREVIOUS = 1 };
int fpc_match_frames(fpc_ctx* ctx, int n, int pairing, const float* key_dev, const int32_t* nkey_dev,
                     int cross_check, float max_dist, float ratio, int32_t* match_dev, float* dist_dev);
int fpc_first_within_frames(fpc_ctx* ctx, int n, const float* key_dev, const int32_t* nkey_dev,
                            float tolerance, int32_t* first_dev);

/* Geometric verification: a RANSAC homography per frame from point correspondences, on the device.  The reference has
 * only the synthesis side (python/src/homographies.py: sample_homography, warp_points, flat2mat, invert_homography); the
 * estimation it would leave to cv2.findHomography(RANSAC), which is not available to this build: the rule below is pinned
 * by planted homographies and by a float64 restatement (tests/test_homography_ransac.py), not against OpenCV.
 *
 * fpc_ransac_homography: explicit correspondences.  src_xy_dev / dst_xy_dev float32 [n][stride][2] (x, y); npairs_dev
 * int32 [n], read on the device and clamped to [0, stride]; 1 <= stride <= fpc_results().capacity; 1 <= n <= max_batch.
 * fpc_homography_frames: straight from the device results of the last call that produced keypoints and a match table
 * of fpc_match_frames (same n, same pairing, same key): the pairs of frame f are (xy[f][i], train_xy[match[f][i]]) for the
 * rows i < count[f] with 0 <= match[f][i] < the train set's row count, in ascending i (other rows are not pairs).
 * train_xy = key_xy_dev int32 [nkey][2] with nkey_dev clamped to [0, cap] (FPC_PAIR_KEY), or xy[f-1] (FPC_PAIR_PREVIOUS;
 * frame 0 against the key, or failing when key_xy_dev is NULL).  Needs no descriptors.
 *
 * Outputs: H_dev float32 [n][9], ninliers_dev int32 [n], inlier_dev uint8 [n][stride] (explicit; indexed by the pair) or
 * [n][cap] (frames; indexed by the query row i), may be NULL.
 *  - Direction: H is row-major with H[8] == 1 and maps a query (src) pixel (x, y, 1) to its train (dst) pixel.
 *  - Inliers: a pair is an inlier of H when |H.src - dst|_2 < reproj_threshold (evaluated without the division, in fp64
 *    from the fp32 H that is returned).  ninliers and inlier are those of the returned H.
 *  - Failure: a frame with fewer than 4 pairs, with no non-degenerate sample, or with fewer than min_inliers inliers after
 *    the last refit gets nine zeros, ninliers = 0 and an all-zero mask.  Mask entries past a frame's pair count (explicit)
 *    or of rows that are not pairs (frames) are 0.
 *  - Sampling: with mix(a): a ^= a >> 16; a *= 0x7feb352d; a ^= a >> 15; a *= 0x846ca68b; a ^= a >> 16 on uint32 (wrapping),
 *    draw k = 0 .. 15 of hypothesis t of frame f over M pairs is
 *        r = mix(seed ^ mix((f * 4096 + t) * 16 + k)) % M.
 *    The draws are taken in order of k; a draw equal to an index already taken is skipped; the first 4 distinct indices
 *    are the sample (in that order), and a hypothesis that has not found 4 within its 16 draws is degenerate.
 *  - Degenerate samples: three of the 4 src or of the 4 dst points collinear (doubled triangle area below 0.5 px^2), a
 *    non-finite H, or an H that cannot be scaled to H[8] = 1 (|h8| <= 1e-12 max|h|).  They score 0 and are never chosen.
 *  - Scoring: the 4-point H is solved exactly in fp64 and applied in fp32; hypothesis t counts the pairs with
 *    |(h1.p, h2.p) - w (u, v)|^2 < threshold^2 w^2 and w = h3.p of the sign it has at the sample's first point.
 *  - Selection: the largest count; ties go to the lower t (an integer maximum: independent of execution order).
 *  - Refit, `refits` times: the inliers of the current H (the rule under "Inliers") are translated to their centroid and
 *    scaled to an RMS distance of sqrt(2), src and dst each (Hartley); the 8 x 8 normal equations of the rows
 *    [x y 1 0 0 0 -ux -uy | u], [0 0 0 x y 1 -vx -vy | v] are summed in fp64 in a fixed order (no floating-point atomics)
 *    and solved by elimination with partial pivoting; the result is denormalised, scaled to H[8] = 1 and rounded to fp32.
 *    Fewer than 4 inliers, a point set of zero spread or a singular system keeps the previous H and ends the refits.
 *  - Determinism: the same seed and the same inputs give bit-identical outputs, and the two entry points give
 *    bit-identical outputs on equal pair lists.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy; may be enqueued right
 *    behind fpc_match_frames and before the next fpc_detect.  The workspace is the ctx's: nothing is allocated per call.
 * FPC_E_INVALID (nothing is written): a NULL ctx / params / input / H_dev / ninliers_dev, iterations outside 1 .. 4096,
 * reproj_threshold not > 0, refits outside 0 .. 4, min_inliers < 4, n < 1, n above max_batch (explicit) or above the
 * frames of the last call that produced keypoints (frames), stride outside 1 .. capacity, a bad pairing, FPC_PAIR_KEY
 * without key_xy_dev, key_xy_dev without nkey_dev. */
typedef struct fpc_ransac_params {
  int      iterations;        /* T hypotheses per frame, 1 .. 4096                                   */
  float    reproj_threshold;  /* pixels, > 0                                                         */
  uint32_t seed;              /* same seed + same inputs -> bit-identical outputs                    */
  int      refits;            /* 0 .. 4 least-squares refits on the inlier set after the best sample */
  int      min_inliers;       /* >= 4; fewer inliers after the last refit -> the frame fails         */
} fpc_ransac_params;
/* 1024 iterations, 3.0 px, seed 0, 2 refits, 8 inliers. */
int fpc_default_ransac_params(fpc_ransac_params* params);
int fpc_ransac_homography(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                          int stride, const fpc_ransac_params* params, float* H_dev, int32_t* ninliers_dev,
                          uint8_t* inlier_dev);
int fpc_homography_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                          const int32_t* match_dev, const fpc_ransac_params* params, float* H_dev, int32_t* ninliers_dev,
                          uint8_t* inlier_dev);

/* --- key-frame bank: a batch against MANY stored key frames in one call (relocalisation, loop closure) ------------------
 * The calls above know one key frame.  The bank keeps up to FPC_BANK_MAX_SLOTS of them on the device -- what 'k' in
 * cpp/src/main.cc:118-123 and 's' in python/src/inference.py:57-60 store, several times over -- and fpc_match_bank answers
 * "which stored frame does this frame see?" for a whole batch without a host round trip; fpc_homography_bank then
 * verifies the answer geometrically.  One bank per ctx.
 *
 * fpc_bank_create: 1 <= slots <= FPC_BANK_MAX_SLOTS, 1 <= rows <= fpc_results().capacity; needs descriptor_enabled.  The
 * ONLY bank call that allocates (and the only one, with fpc_bank_destroy, that synchronises): the storage below, the
 * rows' squared norms and the workspace of fpc_match_bank -- no later bank call allocates.  Every slot starts empty.
 * FPC_E_INVALID when the ctx already has a bank.  fpc_bank_destroy frees it (waiting for the ctx stream first);
 * fpc_destroy frees a bank that is still alive.  In a FPC_PLAN_GUARD_ZONES context every buffer of the bank is followed by
 * a canary zone of its own, and fpc_check_guards counts those too.
 * fpc_bank_get: the bank as device pointers, valid until fpc_bank_destroy / fpc_destroy.  Slot s holds count[s] rows
 * (0 = empty): desc[s][0 .. count[s]) and their pixel coordinates xy[s][..] = (x, y); rows behind count[s] are
 * unspecified.  chunk: the slots one pass of fpc_match_bank scores together (its workspace is max_batch x chunk x
 * capacity entries: DESIGN.md section 7); bytes: everything the bank allocated, that workspace included.
 * fpc_bank_store: frame `frame` of the last call that produced keypoints with descriptors (as for fpc_match_frames) into
 * slot `slot`, replacing what it held: the frame's first min(count[frame], rows) rows -- results are sorted by descending
 * confidence, so with rows < count these are the most confident ones (the rule of cpp/src/main.cc:121-123).  count[frame]
 * is read on the device: the call may be enqueued right behind fpc_detect.  The rows' squared norms are computed here,
 * once, with the partial sums fpc_match_frames uses for its key, which is what makes the distances below bit-equal.
 * fpc_bank_store_rows: the same from caller memory (a saved map): desc_dev [*n][D] fp32, 16-byte aligned, xy_dev [*n][2]
 * int32, *n_dev an int32 in device memory, read on the device and clamped to [0, rows].
 * fpc_bank_clear: count[slot] = 0; slot = -1 clears every slot.
 *
 * fpc_match_bank: the query sets are frames 0 .. n-1 of the last results, as in fpc_match_frames.
 *  - score_dev int32 [n][slots]: score[f][s] = the number of rows i < count[f] for which
 *    fpc_match_frames(frame f, FPC_PAIR_KEY, key = slot s, cross_check, max_dist, ratio) gives match >= 0.  An empty slot
 *    scores 0.  Integer sums: independent of the execution order.
 *  - best_dev int32 [n]: the slot with the largest score, ties to the LOWER slot; -1 when the largest score is below
 *    max(min_score, 1).
 *  - match_dev int32 [n][cap], dist_dev float [n][cap] (both may be NULL): the fpc_match_frames table of frame f against
 *    slot best[f] -- bit-identical to what that call returns with desc[best[f]], count[best[f]] as its key (it IS that
 *    call's kernels, with the key chosen per frame on the device).  A frame with best[f] = -1: -1 / +inf.
 *  - score_dev or best_dev may be NULL, not both.
 *  - Non-finite descriptor rows, in a frame or in a slot: fpc_match's rule on the fp32 d^2 -- such a pair counts in no score
 *    and is no minimum of the table; a slot of non-finite rows scores 0.
 *  - WARNING: a bare cross check (max_dist = 0, ratio = 0) does not discriminate between slots.  Two UNRELATED descriptor
 *    sets have many mutual nearest neighbours (on random unit-norm sets a large share of the smaller set), so an
 *    unrelated slot can outscore the right one.  Give max_dist (the reference's threshold is 0.7, settings.py:6) or a
 *    ratio (0.8), with or without the cross check; tests/test_match_bank.py shows both sides on planted data.
 * fpc_homography_bank: fpc_homography_frames with FPC_PAIR_KEY and a per-frame key: frame f's train coordinates are the
 * bank's xy[slot[f]] with the bank's count[slot[f]]; slot_dev int32 [n] (normally best_dev) is read on the device;
 * match_dev is fpc_match_bank's table.  For every frame the outputs are bit-identical to fpc_homography_frames(n,
 * FPC_PAIR_KEY, xy[slot[f]], &count[slot[f]], match, params) at the SAME frame index (the sampler hashes f).  A frame
 * whose slot is outside [0, slots) -- best = -1 -- has no pairs and fails as under "Failure" above: nine zeros, 0 inliers,
 * an all-zero mask.  Needs no descriptors in the results, only keypoints.
 *
 * All of these but create / destroy: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no
 * allocation; every count is read on the device; deterministic (bit-identical outputs on repeated calls).  A sequence
 * fpc_detect, fpc_bank_store, fpc_detect, fpc_match_bank, fpc_homography_bank needs no host call in between.
 * FPC_E_INVALID (nothing is written): a NULL ctx; no bank (or, for create, a bank already there, descriptor_enabled = 0,
 * slots / rows out of range); slot outside [0, slots) (clear: [-1, slots)); frame outside the frames of the last call
 * that produced keypoints with descriptors; n < 1 or above those frames; results without descriptors (store,
 * match_bank); a NULL or misaligned desc_dev, a NULL xy_dev / n_dev (store_rows); ratio outside [0, 1], max_dist < 0,
 * min_score < 0, score_dev and best_dev both NULL (match_bank); a NULL slot_dev / match_dev / H_dev / ninliers_dev or
 * parameters fpc_homography_frames refuses (homography_bank). */
#define FPC_BANK_MAX_SLOTS 1024
typedef struct fpc_bank_view {
  const float*   desc;    /* [slots][rows][desc_dim]                                   */
  const int32_t* xy;      /* [slots][rows][2]                                          */
  const int32_t* count;   /* [slots], 0 = empty                                        */
  int slots, rows, desc_dim;
  int chunk;              /* slots scored per pass of fpc_match_bank                   */
  size_t bytes;           /* everything the bank allocated, workspace included         */
} fpc_bank_view;
int fpc_bank_create(fpc_ctx* ctx, int slots, int rows);
int fpc_bank_destroy(fpc_ctx* ctx);
int fpc_bank_get(fpc_ctx* ctx, fpc_bank_view* out);
int fpc_bank_store(fpc_ctx* ctx, int frame, int slot);
int fpc_bank_store_rows(fpc_ctx* ctx, int slot, const float* desc_dev, const int32_t* xy_dev, const int32_t* n_dev);
int fpc_bank_clear(fpc_ctx* ctx, int slot);
int fpc_match_bank(fpc_ctx* ctx, int n, int cross_check, float max_dist, float ratio, int min_score, int32_t* score_dev,
                   int32_t* best_dev, int32_t* match_dev, float* dist_dev);
int fpc_homography_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev,
                        const fpc_ransac_params* params, float* H_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);

/* --- epipolar verification: a RANSAC fundamental matrix per frame from the same device-side pair lists ------------------
 * A homography explains two views only of a planar scene or under a pure rotation; a key frame of a room or a street seen
 * from a moved camera supports none.  The other model is the fundamental matrix F with q^T F p = 0 for a query pixel p and
 * its train pixel q.  fpc_ransac_fundamental, fpc_fundamental_frames and fpc_fundamental_bank mirror
 * fpc_ransac_homography, fpc_homography_frames and fpc_homography_bank argument for argument -- the same pair definition,
 * mask indexing, stride rules, fpc_ransac_params, workspace and execution rules (asynchronous on the ctx stream, no host
 * synchronisation, no device-to-host copy, no allocation, every count read on the device) -- with F_dev float32 [n][9] in
 * place of H_dev.  As for the homographies, OpenCV is not available to this build: the rule below is pinned by planted
 * scenes and by a float64 restatement (tests/test_fundamental_ransac.py), not against cv2.findFundamentalMat.
 *  - Direction and form: F is row-major with (u, v, 1) F (x, y, 1)^T = 0, (x, y) the query / src pixel and (u, v) the
 *    train / dst pixel.  F has Frobenius norm 1; its element of largest magnitude (of the fp32 values; ties: the lowest
 *    index) is positive; it has rank 2 up to its fp32 rounding.
 *  - Inliers: with l = F p, l' = F^T q and e = q . l, a pair is an inlier when e^2 < reproj_threshold^2 (l0^2 + l1^2 +
 *    l'0^2 + l'1^2): the Sampson distance below the threshold, without a division, evaluated in fp64 from the fp32 F that
 *    is returned.  ninliers and inlier are those of the returned F.
 *  - Failure: a frame with fewer than 8 pairs, with no non-degenerate sample, or with fewer than min_inliers inliers after
 *    the last refit gets nine zeros, ninliers = 0 and an all-zero mask.
 *  - Sampling: mix() as above with a budget of 32 draws: draw k = 0 .. 31 of hypothesis t of frame f over M pairs is
 *        r = mix(seed ^ mix((f * 4096 + t) * 32 + k)) % M;
 *    a draw equal to an index already taken is skipped; the first 8 distinct indices are the sample (in that order), and a
 *    hypothesis that has not found 8 within its 32 draws is degenerate.
 *  - Minimal solve (8-point), in fp64: the sample's 8 src points are translated to their centroid and scaled to an RMS
 *    distance of sqrt(2), the dst points likewise (a side whose mean squared distance is not > 1e-12 is degenerate).  The
 *    8 x 9 system of the rows [ux uy u vx vy v x y 1] is reduced by Gaussian elimination with FULL pivoting -- the pivot of
 *    step c is the entry of largest magnitude in rows and columns >= c, ties to the lowest row, then the lowest column --
 *    and the null vector is read by back-substitution with the unknown of the last column set to 1: no coordinate of F is
 *    assumed non-zero (a sideways translation has F[8] = 0 exactly).  A last pivot below 1e-10 of the first makes the
 *    sample degenerate (repeated points, rank below 8), so does a non-finite result.  F is denormalised, scaled to
 *    max |f| = 1 and rounded to fp32.  Degenerate samples score 0 and are never chosen.
 *  - Scoring: hypothesis t counts the pairs that pass the Sampson test above in fp32 (fmaf).  Selection: the largest
 *    count; ties go to the lower t (an integer maximum: independent of execution order).
 *  - The best sample's F becomes a returnable F: rank 2 is enforced in the sample's normalised coordinates as
 *    F <- F - (F v3) v3^T, v3 the eigenvector of F^T F's smallest eigenvalue; then it is denormalised, brought to norm 1,
 *    rounded to fp32 and given the sign above.  (In pixel coordinates the projection would be dominated by F[8].)
 *  - Refit, `refits` times: the inliers of the current F are translated and scaled as in the homography refit (the same
 *    moments); M = sum a a^T with a = q (x) p (36 distinct sums) is accumulated in fp64 in a fixed order (no floating-point
 *    atomics); F takes the eigenvector of M's smallest eigenvalue, by cyclic Jacobi with 10 sweeps over (p, q), p < q in
 *    row-major order (rotation: theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)); a zero
 *    a_pq is skipped; the smallest diagonal entry, ties to the lowest index); rank 2 is enforced as above with the same
 *    routine at N = 3; then denormalised, norm 1, fp32, sign.  Fewer than 8 inliers, a point set of zero spread or a
 *    non-finite result keeps the previous F and ends the refits.
 *  - Determinism: as for the homography calls; the three entry points give bit-identical outputs on equal pair lists, and
 *    fpc_fundamental_bank is bit-identical to fpc_fundamental_frames with that slot as key at the SAME frame index.
 *  - Caveat: on a planar scene or under a pure rotation F is not unique.  With measured (rounded, noisy) points, or with
 *    a few outliers among the pairs, the call returns ONE F the pairs agree with.  Pairs that follow a homography EXACTLY
 *    and have no outlier among them (an integer image shift, a frame against itself) leave every 8-point system at rank 6:
 *    every sample is degenerate and the frame FAILS with nine zeros, as under "Failure".  Such scenes are what the
 *    homography calls are for; choosing between the two models is the caller's job.
 * FPC_E_INVALID (nothing is written): everything the homography twin refuses, and min_inliers < 8. */
int fpc_ransac_fundamental(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                           int stride, const fpc_ransac_params* params, float* F_dev, int32_t* ninliers_dev,
                           uint8_t* inlier_dev);
int fpc_fundamental_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                           const int32_t* match_dev, const fpc_ransac_params* params, float* F_dev, int32_t* ninliers_dev,
                           uint8_t* inlier_dev);
int fpc_fundamental_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev,
                         const fpc_ransac_params* params, float* F_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);

/* --- the bank in bf16: half the memory per stored frame, the score pass on the bf16 matrix path --------------------------
 * fpc_bank_create_ex(format): FPC_BANK_F32 is fpc_bank_create, and everything stated above -- every bit-identity with
 * fpc_match_frames included -- holds for it unchanged.  FPC_BANK_BF16 is an opt-in storage AND arithmetic format for
 * ranking slots; an unknown format is FPC_E_INVALID, everything else is as in fpc_bank_create.  One bank per ctx, of one
 * format.  fpc_bank_format: the format, and the descriptors as float* (FPC_BANK_F32) or bf16 bit patterns, uint16_t*
 * (FPC_BANK_BF16), [slots][rows][D]; either output may be NULL, not both.  On a bf16 bank fpc_bank_get gives desc = NULL
 * (no fp32 rows exist); its other fields are as above, and bytes includes the query workspace below.
 *
 * The contract of a FPC_BANK_BF16 bank:
 *  - Store: fpc_bank_store / fpc_bank_store_rows round each fp32 component to bf16, round to nearest even (an overflow
 *    becomes +-inf, a NaN the quiet NaN 0x7FC0, sign and payload dropped); 2 B per component.  norms[slot][row] is
 *    computed in fp32 FROM THE ROUNDED values.  xy and count are as above.
 *  - fpc_match_bank: one pass at the start of the call rounds the n query sets the same way into workspace that
 *    fpc_bank_create_ex allocated (max_batch x capacity x D x 2 B, followed by a canary zone under FPC_PLAN_GUARD_ZONES);
 *    their fp32 norms come from the rounded values.  With q~, t~ the rounded rows
 *        d^2 = max(|q~|^2 + |t~|^2 - 2 q~.t~, 0)
 *    the dot product accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (products of bf16 values are exact in fp32).
 *    Everything behind d^2 is the rule above, by the same code: nearest / second nearest in (d^2 bits, index) order, the
 *    cross check on exact column minima, max_dist, ratio, integer scores, best with ties to the lower slot, min_score.
 *  - The table (match_dev, dist_dev) is computed in the SAME arithmetic against slot best[f]: the number of
 *    match[f][i] >= 0 equals score[f][best[f]] exactly.  It is NOT bit-identical to fpc_match_frames on the fp32 rows:
 *    d^2 differs from the fp32 value by the rounding of the rows (about 1e-3 on unit-norm rows at D = 128), and where two
 *    train rows are closer to each other than that a row may take the other one.
 *  - fpc_match_bank_guided works on it: the gate is the one stated below, a candidate pair's d^2 is the bf16 value above
 *    with the same bits, so with a radius beyond the frame diagonal its output is bit-identical to the fpc_match_bank
 *    table for that slot.  fpc_homography_bank reads xy and count only.  fpc_match_bank, fpc_homography_bank,
 *    fpc_match_bank_guided, fpc_homography_bank needs no host call in between.
 *  - Execution as above: asynchronous on the ctx stream, no allocation after create, no host synchronisation, counts and
 *    slots read on the device.  Deterministic: selection is integer and order-free, the matrix instruction's internal
 *    accumulation order is fixed by the hardware; repeated calls give bit-identical outputs.
 *  - Non-finite descriptor rows: fpc_match's rule, on the fp32 d^2 of the ROUNDED rows (a NaN is stored as 0x7FC0, an
 *    overflow as +-inf): such a pair counts in no score and is no minimum of a table.
 *  - When to use it: to rank slots under max_dist or a ratio (tests/test_match_bank_bf16.py: on planted data the scores and
 *    best equal the fp32 rule's).  The WARNING above about a bare cross check applies, and there the two formats differ. */
#define FPC_BANK_F32  0
#define FPC_BANK_BF16 1
int fpc_bank_create_ex(fpc_ctx* ctx, int slots, int rows, int format);
int fpc_bank_format(fpc_ctx* ctx, int* format, const void** desc);

/* --- guided matching: the match once more, under the estimated homographies as a spatial gate ---------------------------
 * The first pass above is appearance-only: on repetitive texture a row takes a look-alike elsewhere in the image, and
 * RANSAC then discards the pair.  With one H per frame -- what fpc_homography_frames / fpc_homography_bank wrote, passed on
 * unchanged, or under FPC_PAIR_PREVIOUS a motion prior -- the second pass looks only where H sends the row (what
 * python/src/homographies.py's warp_points does on the synthesis side).
 *
 * fpc_match_frames_guided: query sets, train sets, counts, cap and the output shapes are exactly fpc_match_frames' for the
 * same n, pairing, key_dev, nkey_dev.  The train coordinates are fpc_homography_frames': key_xy_dev int32 [nkey][2] for
 * the key (the same nkey_dev), xy[f-1] of the results under FPC_PAIR_PREVIOUS.
 * fpc_match_bank_guided: frame f's train set is the bank's desc[slot[f]], xy[slot[f]], count[slot[f]]; slot_dev int32 [n]
 * (normally fpc_match_bank's best_dev) is read on the device, and a slot outside [0, slots) gives the frame no train rows.
 * H_dev float32 [n][9], row-major, maps a query pixel to its train pixel: the direction and layout the two homography
 * calls write.
 *  - Gate: query row i at the integer pixel (x, y), train row j at (u, v); in fp64 from the fp32 H
 *        w  = H6 x + H7 y + H8
 *        ex = H0 x + H1 y + H2 - w u
 *        ey = H3 x + H4 y + H5 - w v
 *    and row j is a CANDIDATE of row i iff w > 0 and ex^2 + ey^2 < radius^2 w^2 (no division).  A failed frame's nine
 *    zeros give w = 0: no candidates, every row -1 / +inf.  The same holds for an H with any non-finite entry.
 *  - Result: fpc_match_frames' rule over the candidates only: the nearest candidate in (d^2, index) order, dist = its
 *    distance, max_dist and ratio as there with the second-nearest CANDIDATE as d2 (fewer than two candidates: the ratio
 *    test fails).  Cross check: row i survives iff i is the (d^2, index)-nearest among the query rows that have j as a
 *    candidate.  A row without a candidate: -1 / +inf; rows count[f] <= i < cap: -1 / +inf.
 *  - Bits: for a candidate pair d^2 is the value fpc_match_frames computes for that pair (the same norms, K order,
 *    expression and clamp), so where the guided winner equals the unguided winner dist is bit-equal, and with a radius
 *    beyond the frame diagonal (and w > 0 over the frame) the whole output is fpc_match_frames' / the fpc_match_bank table's.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation (the
 *    workspace is fpc_match_frames', carved at fpc_create); every count and slot is read on the device; deterministic
 *    (bit-identical outputs on repeated calls).  fpc_detect, fpc_match_frames, fpc_homography_frames,
 *    fpc_match_frames_guided, fpc_homography_frames needs no host call in between.
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2 -- such a pair is no candidate's minimum, no column minimum,
 * no second best, and a row with no candidate at a finite distance is -1 / +inf.
 * FPC_E_INVALID (nothing is written): everything fpc_match_frames refuses; a NULL H_dev; radius not finite or not > 0;
 * FPC_PAIR_KEY without key_xy_dev; key_dev without key_xy_dev; no bank or a NULL slot_dev (bank variant). */
int fpc_match_frames_guided(fpc_ctx* ctx, int n, int pairing, const float* key_dev, const int32_t* nkey_dev,
                            const int32_t* key_xy_dev, const float* H_dev, float radius, int cross_check, float max_dist,
                            float ratio, int32_t* match_dev, float* dist_dev);
int fpc_match_bank_guided(fpc_ctx* ctx, int n, const int32_t* slot_dev, const float* H_dev, float radius, int cross_check,
                          float max_dist, float ratio, int32_t* match_dev, float* dist_dev);

/* --- cell-ordered guided matching: the guided match, visiting only the tiles the gate can reach ---------------------------
 * fpc_match_frames_guided / fpc_match_bank_guided test the gate against every 64 x 64 tile of (query rows, train rows);
 * rows come in confidence order, so hardly a tile is without a candidate.  The calls below read both sides in a spatial
 * order and skip the tiles whose bounding box no row of the strip can reach within the radius.
 *
 * The order (fpc_cell_order): for a point set of cnt rows with integer pixels (x, y) in a context of frame size H x W,
 *     CX = ceil(W / 32), CY = ceil(H / 32),
 *     cx = clamp(x >> 5, 0, CX - 1), cy = clamp(y >> 5, 0, CY - 1)   (arithmetic shift: rows may lie outside the frame),
 *     cell = cy CX + cx,
 * perm is the stable order by cell: ascending (cell, original index).  fpc_cell_order orders `sets` point sets: set s is
 * xy_dev + s stride 2 (int32 [stride][2]), its count n_dev[s] is read on the device and clamped to [0, stride];
 * perm_dev int32 [sets][stride], entries cnt <= i < stride of a row are unspecified.  It is the kernel the guided calls
 * below run: deterministic (no atomic decides a position), asynchronous on the ctx stream, no allocation.
 * FPC_E_INVALID: a NULL argument, sets < 1, stride < 1, a frame of more than 16384 cells (16.7 MPx).
 *
 * fpc_match_frames_guided_cells / fpc_match_bank_guided_cells: the arguments of fpc_match_frames_guided /
 * fpc_match_bank_guided plus stats_dev.
 *  - For every argument set those calls accept, match_dev and dist_dev are BIT-IDENTICAL to what they write: indices are
 *    original row indices; rows past the count, frames without a train set, slots outside the bank and empty slots, a
 *    zero or non-finite H and w <= 0 included.  (The result is a function of the candidate set and of each candidate
 *    pair's d^2 bits: nearest and second nearest are the two smallest (d^2 bits, index) keys, the column minimum the
 *    smallest, whatever order rows are visited in.  In a frame of more than 16384 cells the calls order by coarser
 *    cells; the output is the same.)
 *  - stats_dev int32 [n][2], or NULL: per frame {(strip, tile) pairs visited, strips x tiles where both sets are
 *    non-empty}, a strip being 64 ordered query rows and a tile 64 ordered train rows.  Deterministic.
 *  - Execution: as for the existing calls -- asynchronous on the ctx stream, no host synchronisation, no copy, no
 *    allocation (orders and boxes live in the workspace carved at fpc_create; nothing is added to the bank's allocation),
 *    every count and slot read on the device.  fpc_match_frames, fpc_homography_frames, fpc_match_frames_guided_cells,
 *    fpc_homography_frames needs no host call in between.  Per call: the order of the query sets (frames 0 .. n-1) and of
 *    the train sets (the key once; under FPC_PAIR_PREVIOUS frame f-1's query order is reused; the slot of every frame).
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2 -- such a pair is no candidate's minimum, no column minimum,
 * no second best, and a row with no candidate at a finite distance is -1 / +inf.
 * FPC_E_INVALID (nothing is written, stats_dev included): everything fpc_match_frames_guided / fpc_match_bank_guided
 * refuse; the bank variant on a FPC_BANK_BF16 bank (that format's ordered strip is the follow-up). */
int fpc_cell_order(fpc_ctx* ctx, const int32_t* xy_dev, const int32_t* n_dev, int sets, int stride, int32_t* perm_dev);
int fpc_match_frames_guided_cells(fpc_ctx* ctx, int n, int pairing, const float* key_dev, const int32_t* nkey_dev,
                                  const int32_t* key_xy_dev, const float* H_dev, float radius, int cross_check,
                                  float max_dist, float ratio, int32_t* match_dev, float* dist_dev, int32_t* stats_dev);
int fpc_match_bank_guided_cells(fpc_ctx* ctx, int n, const int32_t* slot_dev, const float* H_dev, float radius,
                                int cross_check, float max_dist, float ratio, int32_t* match_dev, float* dist_dev,
                                int32_t* stats_dev);

/* --- epipolar guided matching: the match once more, under the estimated fundamental matrices as the gate ------------------
 * The guided calls above close the loop for scenes a homography explains.  For the other model -- a room or a street seen
 * from a moved camera, fpc_fundamental_frames / fpc_fundamental_bank -- the gate is a band around the epipolar line: with
 * one F per frame, what those calls wrote, passed on unchanged, the second pass looks only along the line F gives the row.
 *
 * fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar: the arguments of fpc_match_frames_guided /
 * fpc_match_bank_guided, argument for argument, with F_dev float32 [n][9] where H_dev stands.  Query sets, train sets, train
 * coordinates, counts, cap, the output shapes, the pairing, the key rules and the slot rules are those calls', unchanged.
 *  - F is row-major with (u, v, 1) F (x, y, 1)^T = 0, (x, y) the query pixel and (u, v) the train pixel: the direction and
 *    layout the three fundamental calls write.
 *  - Gate: query row i at the integer pixel p = (x, y, 1), train row j at q = (u, v, 1); in fp64 from the fp32 F
 *        l  = F p
 *        l' = F^T q
 *        e  = q . l = l0 u + l1 v + l2
 *    and row j is a CANDIDATE of row i iff e^2 < radius^2 (l0^2 + l1^2 + l'0^2 + l'1^2): the Sampson distance below the
 *    radius.  This is the inlier test of fpc_ransac_fundamental with radius in the place of reproj_threshold: a pair that a
 *    fundamental call marks as an inlier at threshold t is a candidate at radius t.  No division and no sign condition (a
 *    line has no "behind the camera"): F and -F give the same output.  A failed frame's nine zeros give 0 < 0: no
 *    candidates, every row -1 / +inf.  The same holds for an F with any non-finite entry.
 *  - Result: fpc_match_frames' rule over the candidates only: the nearest candidate in (d^2, index) order, dist = its
 *    distance, max_dist and ratio as there with the second-nearest CANDIDATE as d2 (fewer than two candidates: the ratio
 *    test fails).  Cross check: row i survives iff i is the (d^2, index)-nearest among the query rows that have j as a
 *    candidate.  A row without a candidate: -1 / +inf; rows count[f] <= i < cap: -1 / +inf.
 *  - Bits: for a candidate pair d^2 is the value fpc_match_frames computes for that pair (the same norms, K order,
 *    expression and clamp), so where the guided winner equals the unguided winner dist is bit-equal, and under a radius at
 *    which EVERY pair of a frame is a candidate the frame's output is fpc_match_frames' / the fpc_match_bank table's, bit
 *    for bit.  Unlike the homography gate, no fixed radius guarantees that for every F: the epipolar line of a pixel need
 *    not cross the frame, so the radius that admits every pair depends on F.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation (the
 *    workspace is fpc_match_frames', carved at fpc_create; nothing new is carved, the plan hash and the guard zones are what
 *    they were); every count and slot is read on the device; deterministic (bit-identical outputs on repeated calls).
 *    fpc_detect, fpc_match_frames, fpc_fundamental_frames, fpc_match_frames_guided_epipolar, fpc_fundamental_frames needs no
 *    host call in between; the same holds through the bank with fpc_match_bank, fpc_fundamental_bank,
 *    fpc_match_bank_guided_epipolar, fpc_fundamental_bank.
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2 -- such a pair is no candidate's minimum, no column minimum,
 * no second best, and a row with no candidate at a finite distance is -1 / +inf.
 * FPC_E_INVALID (nothing is written): everything fpc_match_frames_guided / fpc_match_bank_guided refuse, with F_dev for
 * H_dev; the bank variant on a FPC_BANK_BF16 bank (that format's epipolar gate is the follow-up). */
int fpc_match_frames_guided_epipolar(fpc_ctx* ctx, int n, int pairing, const float* key_dev, const int32_t* nkey_dev,
                                     const int32_t* key_xy_dev, const float* F_dev, float radius, int cross_check,
                                     float max_dist, float ratio, int32_t* match_dev, float* dist_dev);
int fpc_match_bank_guided_epipolar(fpc_ctx* ctx, int n, const int32_t* slot_dev, const float* F_dev, float radius,
                                   int cross_check, float max_dist, float ratio, int32_t* match_dev, float* dist_dev);

/* --- cell-ordered epipolar guided matching: the epipolar match, visiting only the tiles the bands can reach ---------------
 * fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar test the gate against every 64 x 64 tile of (query rows,
 * train rows); rows come in confidence order, so every tile has a pair inside some row's band and none is skipped.  The calls
 * below read both sides in fpc_cell_order's spatial order and skip the tiles whose bounding box no band of the strip can
 * reach: what the cell-ordered calls above do for the homography gate, for the epipolar one.
 *
 * fpc_match_frames_guided_epipolar_cells / fpc_match_bank_guided_epipolar_cells: the arguments of
 * fpc_match_frames_guided_cells / fpc_match_bank_guided_cells, argument for argument, with F_dev where H_dev stands.
 *  - Output: for every argument set fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar accept, match_dev and
 *    dist_dev are BIT-IDENTICAL to what they write: indices are original row indices; rows past the count, frames without a
 *    train set, slots outside the bank and empty slots, nine zeros, a non-finite F, and F versus -F included.  (The result
 *    is a function of the candidate set and of each candidate pair's d^2 bits, whatever order rows are visited in.)
 *  - stats_dev int32 [n][2], or NULL, with the meaning of the cell-ordered calls above: per frame {(strip, tile) pairs
 *    visited, strips x tiles where both sets are non-empty}, a strip being 64 ordered query rows and a tile 64 ordered train
 *    rows.  Deterministic.
 *  - Order: the order and the boxes are fpc_cell_order's -- the same kernel, the same coarser cells in a frame of more than
 *    16384 cells, the same workspace.  Per call: the order of the query sets (frames 0 .. n-1) and of the train sets (the
 *    key once; under FPC_PAIR_PREVIOUS frame f-1's query order serves as the train order; the slot of every frame).
 *  - Cull: with l = F p and g = l0^2 + l1^2 of the gate above for a query row (g = -inf for a row that passes nowhere: a row
 *    past the count, a non-finite F), and a train tile whose 64 ordered rows have the pixel box [u0, u1] x [v0, v1]:
 *        e_lo, e_hi = the minimum and the maximum of l0 u + l1 v + l2 over the four corners of the box
 *                     (e is linear: this is its exact range over the box),
 *        m  = 0 if e_lo <= 0 <= e_hi, else min(|e_lo|, |e_hi|),
 *        G  = max over the four corners of l'0^2 + max over the four corners of l'1^2,  l' = F^T (u, v, 1)
 *             (once per tile, the same for every row),
 *    the row can reach the tile iff m^2 < radius^2 (g + G), and a strip visits a tile iff one of its rows can reach it.
 *    Every candidate pair has |e| >= m and l'0^2 + l'1^2 <= G, so no tile that holds a candidate is dropped; the device
 *    evaluates the rule in fp64 with e_lo, e_hi and the range of l' widened by a few units in the last place, which makes
 *    this hold for the gate as the device computes it, whichever way its sums are fused.
 *  - Execution: as for the twins -- asynchronous on the ctx stream, no host synchronisation, no copy, no allocation, every
 *    count and slot read on the device.  Nothing new is carved: orders and boxes live in the workspace of the cell-ordered
 *    calls above, the plan hash and the guard zones are what they were, nothing is added to the bank's allocation.
 *    fpc_match_frames, fpc_fundamental_frames, fpc_match_frames_guided_epipolar_cells, fpc_fundamental_frames needs no host
 *    call in between; the same holds through the bank with fpc_match_bank, fpc_fundamental_bank,
 *    fpc_match_bank_guided_epipolar_cells, fpc_fundamental_bank.
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2 -- such a pair is no candidate's minimum, no column minimum,
 * no second best, and a row with no candidate at a finite distance is -1 / +inf.
 * FPC_E_INVALID (nothing is written, stats_dev included): everything fpc_match_frames_guided_epipolar /
 * fpc_match_bank_guided_epipolar refuse; the bank variant on a FPC_BANK_BF16 bank (that format's strip is the follow-up). */
int fpc_match_frames_guided_epipolar_cells(fpc_ctx* ctx, int n, int pairing, const float* key_dev, const int32_t* nkey_dev,
                                           const int32_t* key_xy_dev, const float* F_dev, float radius, int cross_check,
                                           float max_dist, float ratio, int32_t* match_dev, float* dist_dev,
                                           int32_t* stats_dev);
int fpc_match_bank_guided_epipolar_cells(fpc_ctx* ctx, int n, const int32_t* slot_dev, const float* F_dev, float radius,
                                         int cross_check, float max_dist, float ratio, int32_t* match_dev, float* dist_dev,
                                         int32_t* stats_dev);

/* --- verified relocalisation: the K best slots of the bank per frame, each checked by RANSAC -----------------------------
 * fpc_match_bank ranks the slots by appearance and returns ONE per frame; everything behind it verifies that slot.  Where a
 * look-alike slot outscores the right one (the WARNING above; repetitive texture, revisited places) the homography fails and
 * the frame is lost although the right slot came second.  The calls below shortlist the k best slots, estimate a homography
 * against each of them, and keep the slot with the most inliers -- without a host loop over the candidates.
 *
 * fpc_bank_topk_reserve: 1 <= kmax <= min(FPC_BANK_TOPK_MAX, slots); needs a bank.  The ONLY call of the three that
 * allocates or synchronises: workspace for max_batch x kmax (frame, candidate) pairs -- top-2 keys [max_batch][kmax][cap][2],
 * column minima [max_batch][kmax][rows], the candidate tables, and the RANSAC pair lists, rows, counts and best keys of
 * max_batch x kmax problems -- in an allocation of its own.  *bytes (may be NULL) receives its size; fpc_bank_get().bytes
 * and chunk, fpc_create's workspace and the bank are what they were.  FPC_E_INVALID without a bank or when a reservation
 * already exists; fpc_bank_destroy and fpc_destroy free it.  In a FPC_PLAN_GUARD_ZONES context every buffer of it is
 * followed by a canary zone of its own, and fpc_check_guards counts those too.
 *
 * fpc_match_bank_topk: 1 <= k <= kmax; the query sets are frames 0 .. n-1 of the last results, on either bank format.
 *  - score_dev int32 [n][slots] (may be NULL): fpc_match_bank's score, computed by the same passes: the same integers.
 *  - cand_slot_dev int32 [n][k]: cand_slot[f][j] is the j-th slot in descending (score, then LOWER slot first) order among
 *    the slots with score >= max(min_score, 1); entries behind the last such slot are -1.  cand_slot[f][0] is
 *    fpc_match_bank's best[f].  An integer selection: no atomic decides a position.
 *  - cand_score_dev int32 [n][k] (may be NULL): the scores of those slots; 0 where the slot is -1.
 *  - match_dev int32 [n][k][cap], dist_dev float [n][k][cap] (both may be NULL): match[f][j] / dist[f][j] is the table of
 *    frame f against slot cand_slot[f][j] in the bank's arithmetic -- bit-identical to what fpc_match_bank_guided writes
 *    for that frame with that slot, an identity H and a radius beyond the frame diagonal, which is the fpc_match_bank table
 *    for that slot on either format and, on a FPC_BANK_F32 bank, fpc_match_frames with the slot as its key.  The number of
 *    match[f][j][i] >= 0 equals cand_score[f][j].  A candidate of -1: -1 / +inf rows.
 * fpc_homography_bank_topk: one RANSAC problem per (frame, candidate).  cand_slot_dev [n][k] and match_dev [n][k][cap] are
 * fpc_match_bank_topk's; H_dev float32 [n][k][9], ninliers_dev int32 [n][k], inlier_dev uint8 [n][k][cap] (may be NULL).
 *  - Problem (f, j) is bit-identical to fpc_homography_bank(n, slot = cand_slot[.][j], match = match[.][j], params) at
 *    frame index f -- H, ninliers and the mask, failed frames and candidates of -1 (nine zeros, 0, an all-zero mask)
 *    included: the sampler hashes f, not f k + j.
 *  - pick_dev int32 [n] (may be NULL): the j with the largest ninliers[f][j], ties to the LOWER j; -1 when every
 *    ninliers[f][.] is 0.  best_dev int32 [n] (may be NULL): cand_slot[f][pick[f]], or -1.  The integer key
 *    (ninliers << 32) | ~j: independent of the execution order.
 *  - Needs keypoints only, as fpc_homography_bank.
 * Execution: both calls are asynchronous on the ctx stream, with no host synchronisation, no device-to-host copy and no
 * allocation; counts and slots are read on the device; repeated calls give bit-identical outputs.  The number of launches of
 * a call does not depend on n or k (the score pass loops over the bank's slot chunks, as in fpc_match_bank).  fpc_detect,
 * fpc_match_bank_topk, fpc_homography_bank_topk, fpc_match_bank_guided(best), fpc_homography_bank(best) needs no host call
 * in between.
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2, in the scores and in every candidate's table.
 * FPC_E_INVALID (nothing is written): everything fpc_match_bank (but a NULL score_dev) / fpc_homography_bank refuses; no
 * reservation; k outside [1, kmax]; a NULL cand_slot_dev; a NULL match_dev / H_dev / ninliers_dev (homography call). */
#define FPC_BANK_TOPK_MAX 16
int fpc_bank_topk_reserve(fpc_ctx* ctx, int kmax, size_t* bytes);
int fpc_match_bank_topk(fpc_ctx* ctx, int n, int k, int cross_check, float max_dist, float ratio, int min_score,
                        int32_t* score_dev, int32_t* cand_slot_dev, int32_t* cand_score_dev, int32_t* match_dev,
                        float* dist_dev);
int fpc_homography_bank_topk(fpc_ctx* ctx, int n, int k, const int32_t* cand_slot_dev, const int32_t* match_dev,
                             const fpc_ransac_params* params, float* H_dev, int32_t* ninliers_dev, uint8_t* inlier_dev,
                             int32_t* pick_dev, int32_t* best_dev);

/* --- relative pose: R, t and triangulated points from a fundamental matrix and the pairs behind it ------------------------
 * The fundamental calls end in an F and an inlier mask; a tracker, a relocaliser or a mapper wants where the camera moved
 * and where the points are.  With the intrinsics of the two cameras, fpc_pose_fundamental, fpc_pose_frames and fpc_pose_bank
 * turn one F per frame -- what fpc_ransac_fundamental / fpc_fundamental_frames / fpc_fundamental_bank wrote, passed on
 * unchanged -- into a rotation, a translation direction and one 3-D point per pair, on the device.  They mirror those three
 * calls argument for argument: the same pair definition, strides, clamping of counts, pairing, key and slot rules, workspace
 * and execution rules, with F_dev float32 [n][9] as an INPUT and fpc_pose_params in the place of fpc_ransac_params.
 * Outputs: R_dev float32 [n][9] row-major, t_dev float32 [n][3], nfront_dev int32 [n], xyz_dev float32 [n][S][3] (may be
 * NULL), front_dev uint8 [n][S] (may be NULL); S is `stride` for fpc_pose_fundamental and the capacity for the other two,
 * and a row of xyz / front is a pair (fpc_pose_fundamental) or a query row (frames, bank), as for the inlier masks.
 *  - Convention: X_train = R X_query + t with det R = +1 and |t| = 1: the scale of a translation is unobservable from two
 *    views.  The points are in the query camera's frame, at that scale.
 *  - Pairs used: the pairs of the list that pass the Sampson test of the fundamental section above with this struct's
 *    reproj_threshold, evaluated in fp64 from the fp32 F.  With the threshold F was estimated with, these are exactly the
 *    pairs of that call's mask.
 *  - Essential matrix: with K = [fx 0 cx; 0 fy cy; 0 0 1] of either side, E = K_t^T F K_q in fp64, scaled to max |e| = 1.
 *  - Decomposition: A = E^T E is diagonalised by the cyclic Jacobi of the fundamental section at N = 3 (10 sweeps, the same
 *    rotation rule).  i1, i2 are the indices of the two largest diagonal entries, in descending order, ties to the lowest
 *    index, lambda1 >= lambda2 those entries; the frame fails unless lambda2 > 1e-12 lambda1.  v1, v2 are the eigenvectors
 *    (columns i1, i2), v3 = v1 x v2; u1 = E v1 / |E v1|; u2 = E v2 with its u1 component removed, then normalised;
 *    u3 = u1 x u2;
 *        R_a =  u2 v1^T - u1 v2^T + u3 v3^T,      R_b = -u2 v1^T + u1 v2^T + u3 v3^T,
 *    and the four candidates are c = 0 .. 3 = (R_a, +u3), (R_a, -u3), (R_b, +u3), (R_b, -u3).
 *  - Triangulation (midpoint), per used pair and candidate (R, t), in fp64: p^ = ((x - q_cx) / q_fx, (y - q_cy) / q_fy, 1)
 *    for the query pixel, q^ likewise from the train pixel and the train intrinsics; a = R p^, b = q^,
 *        det = (a.a)(b.b) - (a.b)^2,
 *        lam = ((a.b)(b.t) - (a.t)(b.b)) / det,      mu = ((a.a)(b.t) - (a.b)(a.t)) / det
 *    (the parameters at which the rays lam a + t and mu b are closest).  The pair is IN FRONT under the candidate when
 *    det > 1e-12 (a.a)(b.b) and lam > 0 and mu > 0.
 *  - Selection: the candidate with the most pairs in front; ties go to the lower c.  The counts are integers, so the result
 *    does not depend on the execution order.
 *  - Outputs: nfront is that count; front[row] = 1 for the chosen candidate's pairs in front and 0 elsewhere -- pairs that
 *    are not used, rows past the count and rows that are no pair included; xyz[row] = (lam p^ + R^T (mu q^ - t)) / 2, the
 *    midpoint of the two closest points, for those pairs and three zeros elsewhere.  R and t are rounded to fp32.  The
 *    call writes every row of its frames' front / xyz: nothing needs to be cleared beforehand.
 *  - Failure: an all-zero F (a failed frame of the fundamental calls) or one with a non-finite entry, no pair used, a failed
 *    rank test, a non-finite R or t, or nfront < min_front: nine zeros, three zeros, nfront = 0, an all-zero front and an
 *    all-zero xyz.  A bank slot outside [0, slots) leaves the frame without pairs and fails the same way.
 *  - Which candidate gets which index c: for a true essential matrix lambda1 = lambda2, and for an estimated one nearly so;
 *    the eigenvector basis (v1, v2) of that plane is then arbitrary (it is whatever the Jacobi sweeps arrive at).  A
 *    rotation of the basis within its plane changes nothing; an odd permutation (v1 <-> v2) swaps the labels R_a <-> R_b
 *    and the sign of u3.  The SET of four candidates, and with it the selected pose, nfront, front and xyz, is invariant;
 *    the index c of a candidate, and so the outcome of an exact tie between two candidates, is not.  A tie between
 *    candidates that both reach min_front does not arise from a scene with depth: a point in front of both cameras under
 *    one candidate is behind one of them under the other three.
 *  - Workspace: the calls run the fundamental calls' pack / gather kernels (without a mask: nothing of the caller's is
 *    zeroed) into the same pair-list workspace, so a pose call replaces the previous RANSAC call's pair list by an equal
 *    one.  Nothing new is carved; the plan hash and the guard zones are what they were.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation; every count
 *    and slot is read on the device.  fpc_match_frames, fpc_fundamental_frames, fpc_pose_frames needs no host call in
 *    between; the same holds through the bank with fpc_match_bank, fpc_fundamental_bank, fpc_pose_bank.
 *  - Determinism: bit-identical outputs on repeated calls (no floating-point atomics; the counts are sums of 0 / 1); the
 *    three entry points give bit-identical outputs on equal pair lists, and fpc_pose_bank is bit-identical to
 *    fpc_pose_frames with that slot as key.
 * FPC_E_INVALID (nothing is written): everything the fundamental twin refuses for the arguments they share; a NULL F_dev /
 * params / R_dev / t_dev / nfront_dev; fx or fy not > 0 or any non-finite intrinsic; reproj_threshold not > 0 (or not
 * below 1e18); min_front < 1. */
typedef struct fpc_pose_params {
  float q_fx, q_fy, q_cx, q_cy;   /* intrinsics of the query camera (pixels), fx, fy > 0                                  */
  float t_fx, t_fy, t_cx, t_cy;   /* intrinsics of the train camera                                                       */
  float reproj_threshold;         /* px, > 0: which pairs count (the Sampson rule of fpc_ransac_fundamental)              */
  int   min_front;                /* >= 1; fewer pairs in front of both cameras -> the frame fails                        */
} fpc_pose_params;
/* fx = fy = 500, centre (320, 240) on both sides, reproj_threshold 3.0, min_front 8 */
int fpc_default_pose_params(fpc_pose_params* params);
int fpc_pose_fundamental(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                         int stride, const float* F_dev, const fpc_pose_params* params, float* R_dev, float* t_dev,
                         int32_t* nfront_dev, float* xyz_dev, uint8_t* front_dev);
int fpc_pose_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                    const int32_t* match_dev, const float* F_dev, const fpc_pose_params* params, float* R_dev, float* t_dev,
                    int32_t* nfront_dev, float* xyz_dev, uint8_t* front_dev);
int fpc_pose_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const float* F_dev,
                  const fpc_pose_params* params, float* R_dev, float* t_dev, int32_t* nfront_dev, float* xyz_dev,
                  uint8_t* front_dev);

/* --- relative pose from a homography: planar scenes and pure rotations -------------------------------------------------------
 * The caveat of the fundamental section is this section's case: a wall, a floor, a desk, a poster, or a camera that turns on
 * the spot has no unique F, and the homography calls end in an H and a mask.  fpc_pose_homography,
 * fpc_pose_homography_frames and fpc_pose_homography_bank turn one H per frame -- what fpc_ransac_homography /
 * fpc_homography_frames / fpc_homography_bank wrote, passed on unchanged -- into rotations, translation directions, the
 * plane and one 3-D point per pair, on the device.  They mirror those three calls argument for argument: the same pair
 * definition, strides, clamping of counts, pairing, key and slot rules, workspace and execution rules, with H_dev float32
 * [n][9] as an INPUT and fpc_pose_homography_params in the place of fpc_ransac_params.
 * Outputs (S is `stride` for fpc_pose_homography and the capacity for the other two; a row of xyz / front is a pair
 * (fpc_pose_homography) or a query row (frames, bank), as for fpc_pose_*):
 *    kind_dev    int32   [n]        FPC_POSE_H_FAILED, FPC_POSE_H_UNIQUE, FPC_POSE_H_TWOFOLD or FPC_POSE_H_ROTATION
 *    R_dev       float32 [n][2][9]  row-major; X_train = R X_query + t, det R = +1
 *    t_dev       float32 [n][2][3]  |t| = 1
 *    plane_dev   float32 [n][2][4]  may be NULL; (N, d): the plane N.X = d in the query camera's frame, |N| = 1, d > 0, at
 *                                   the scale where |t| = 1
 *    nfront_dev  int32   [n][2]     the support count defined below
 *    nplane_dev  int32   [n][2]     may be NULL; a candidate's H inliers in front
 *    xyz_dev     float32 [n][S][3]  may be NULL; the points of solution `which`, in fpc_pose_*'s format
 *    front_dev   uint8   [n][S]     may be NULL; likewise
 * xyz[f] and front[f] go into fpc_bank_store_landmarks as they are.  Solution 0 is the better one; a solution that does not
 * exist is all zeros.  Everything is evaluated in fp64 from the fp32 H; only R, t, the plane and xyz are rounded to fp32.
 *  - Normalisation: with K = [fx 0 cx; 0 fy cy; 0 0 1] of either side, H^ = K_t^-1 H K_q, written out for that K (H K_q
 *    column by column, then rows 0 and 1 less cx, cy times row 2 and divided by fx, fy), scaled to max |h^| = 1.  A zero H
 *    (a failed frame of the homography calls), a non-finite H, a frame with no pairs, or a bank slot outside [0, slots)
 *    fails the frame.
 *  - Eigen-decomposition: S = H^T H^ is diagonalised by the cyclic Jacobi of the fundamental section at N = 3 (10 sweeps,
 *    the same rotation rule).  lambda1 >= lambda2 >= lambda3 are the diagonal entries in descending order, ties to the
 *    lowest index, as the pose call picks its two; v1, v2 are their columns and v3 = v1 x v2.  The frame fails unless
 *    lambda3 > 1e-12 lambda1.  Then H^ <- H^ / sqrt(lambda2) and lambda_i <- lambda_i / lambda2; if det H^ < 0, H^ <- -H^,
 *    which puts both cameras on one side of the plane.
 *  - Baseline: b = sqrt(lambda1) - sqrt(lambda3); for H = R + T N^T / d this is |T| / d, the baseline over the plane's
 *    distance.  b <= min_baseline makes the frame a pure rotation: kind = FPC_POSE_H_ROTATION, solution 0's R =
 *    w1 v1^T + w2 v2^T + w3 v3^T with w1 = H^ v1 / |H^ v1|, w2 = H^ v2 with its w1 component removed, then normalised, and
 *    w3 = w1 x w2; everything else of the frame is zero (a non-finite R fails the frame).
 *  - Candidates (the four-solution form of Ma, Soatto, Kosecka and Sastry, An Invitation to 3-D Vision, section 5.3): with
 *    a = sqrt(max(0, 1 - lambda3)), c = sqrt(max(0, lambda1 - 1)) and e = sqrt(lambda1 - lambda3),
 *        u+- = (a v1 +- c v3) / e,
 *    and for each sign U = [v2, u, v2 x u], W = [H^ v2, H^ u, H^ v2 x H^ u] (columns),
 *        R = W U^T,      N = v2 x u,      T = (H^ - R) N.
 *    The four candidates are c = 0 .. 3 = (R+, T+, N+), (R+, -T+, -N+), (R-, T-, N-), (R-, -T-, -N-), with t = T / |T| and
 *    d = 1 / |T|.  A candidate with a non-finite value is dropped.
 *  - Counting, per candidate, over ALL pairs of the list: triangulation and the IN FRONT test are those of fpc_pose_*,
 *    unchanged.  nplane_c counts the pairs that are inliers of H by the homography section's "Inliers" rule at this
 *    struct's reproj_threshold and are in front.  nfront_c, the support, counts the pairs that are in front and pass the
 *    Sampson rule of the fundamental section at the same threshold under
 *        F_c = K_t^-T [t]x R K_q^-1
 *    (E = [t]x R; its columns divided by q_fx, q_fy and the third less q_cx, q_cy times those; then its rows likewise with
 *    the train camera).  Plane pairs satisfy that rule by construction (H.p lies on p's epipolar line); pairs off the
 *    plane satisfy it only under the true motion.
 *  - Selection: candidates with nplane_c < min_front are dropped; the rest are ranked by the integer key
 *    (nfront_c << 32) | ~c, and solutions 0 and 1 are the two largest.  kind is UNIQUE when one candidate remains, TWOFOLD
 *    when two or more remain, FAILED when none does.  front[row] = 1 for solution `which`'s support pairs, xyz[row] is
 *    their midpoint (the formula of fpc_pose_*), zeros everywhere else; the call writes every row of its frames' front /
 *    xyz.
 *  - The twofold ambiguity is a property of planes, not of this code.  Cheirality removes the two -T candidates; the other
 *    two both keep every plane point in front unless some point violates N.x > 0 for one of them.  In a float64 check of
 *    this rule on 300 planted VGA scenes (K = (500, 500, 320, 240), planes at depth 4 - 8 tilted up to 50 degrees,
 *    rotations of 3 - 20 degrees, baselines of 0.1 - 0.5 plane distances, integer pixels, 3 px) the two survivors tied on
 *    support in 56 % of the scenes when every pair lay on the plane, and the pick between them was wrong in about a third
 *    of all scenes.  With 5 % of the pairs off the plane the tie rate fell to 1.7 % and the wrong picks to 0.7 %; with 15 %
 *    there were 0 wrong picks in 297 scenes.  So the call always returns both survivors and their counts, and what
 *    nfront[1] against nfront[0] means is the caller's decision; a third view through fpc_pnp_* against either solution's
 *    points also settles it.
 *  - Which candidate gets which index c: v1, v2 are determined up to their signs (and, where two lambdas meet, up to a
 *    rotation).  Negating v1 swaps c = 0 <-> 1 and 2 <-> 3; negating v2 swaps 0 <-> 3 and 1 <-> 2.  The SET of four
 *    candidates is invariant; the index c of a candidate, and so the outcome of an exact tie between two candidates, is
 *    not -- as for fpc_pose_*.
 *  - Workspace, execution and determinism are fpc_pose_*'s: the calls run the homography calls' pack / gather kernels
 *    (without a mask: nothing of the caller's is zeroed) into the same pair-list workspace; nothing new is carved or
 *    allocated, the plan hash and the guard zones are what they were; asynchronous on the ctx stream, no host
 *    synchronisation, no device-to-host copy, every count and slot read on the device, so fpc_match_bank,
 *    fpc_homography_bank, fpc_pose_homography_bank, fpc_bank_store + fpc_bank_store_landmarks needs no host call in
 *    between; bit-identical outputs on repeated calls; the three entry points give bit-identical outputs on equal pair
 *    lists, and fpc_pose_homography_bank is bit-identical to fpc_pose_homography_frames with that slot as key.
 * FPC_E_INVALID (nothing is written): everything the homography twin refuses for the arguments they share; a NULL H_dev /
 * params / kind_dev / R_dev / t_dev / nfront_dev; fx or fy not > 0 or any non-finite intrinsic; reproj_threshold not > 0
 * (or not below 1e18); min_front < 1; min_baseline negative or not finite; which outside 0 .. 1. */
enum { FPC_POSE_H_FAILED = 0, FPC_POSE_H_UNIQUE = 1, FPC_POSE_H_TWOFOLD = 2, FPC_POSE_H_ROTATION = 3 };
typedef struct fpc_pose_homography_params {
  float q_fx, q_fy, q_cx, q_cy;   /* intrinsics of the query camera (pixels), fx, fy > 0                                  */
  float t_fx, t_fy, t_cx, t_cy;   /* intrinsics of the train camera                                                       */
  float reproj_threshold;         /* px, > 0: which pairs count (plane pairs: the homography rule; support: Sampson)      */
  int   min_front;                /* >= 1; a candidate with fewer plane pairs in front is dropped                         */
  float min_baseline;             /* >= 0; baseline over plane distance at or below which the frame is a pure rotation    */
  int   which;                    /* 0 or 1: the solution whose points go to xyz / front                                  */
} fpc_pose_homography_params;
/* fpc_default_pose_params' cameras and reproj_threshold, min_front 8, min_baseline 0.01, which 0 */
int fpc_default_pose_homography_params(fpc_pose_homography_params* params);
int fpc_pose_homography(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                        int stride, const float* H_dev, const fpc_pose_homography_params* params, int32_t* kind_dev,
                        float* R_dev, float* t_dev, float* plane_dev, int32_t* nfront_dev, int32_t* nplane_dev,
                        float* xyz_dev, uint8_t* front_dev);
int fpc_pose_homography_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                               const int32_t* match_dev, const float* H_dev, const fpc_pose_homography_params* params,
                               int32_t* kind_dev, float* R_dev, float* t_dev, float* plane_dev, int32_t* nfront_dev,
                               int32_t* nplane_dev, float* xyz_dev, uint8_t* front_dev);
int fpc_pose_homography_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const float* H_dev,
                             const fpc_pose_homography_params* params, int32_t* kind_dev, float* R_dev, float* t_dev,
                             float* plane_dev, int32_t* nfront_dev, int32_t* nplane_dev, float* xyz_dev, uint8_t* front_dev);

/* --- absolute pose from bank landmarks: RANSAC perspective-n-point on the device ------------------------------------------
 * fpc_pose_* ends in a translation DIRECTION: two views cannot give its scale, so every relocalisation comes back at a scale
 * of its own.  The triangulated points it writes remove that limit.  They are indexed by the query row, which is the row
 * order fpc_bank_store keeps for the same frame; once a stored key frame carries its 3-D points (landmarks), a later frame
 * that matches that slot has 2-D <-> 3-D pairs, and perspective-n-point on those gives R and t at the map's scale from ONE
 * view -- also where the baseline to the key frame is too short for an F.  fpc_ransac_pnp, fpc_pnp_frames and fpc_pnp_bank
 * mirror fpc_ransac_fundamental, fpc_fundamental_frames and fpc_fundamental_bank: explicit pairs, the frames of the last
 * detect against one key set, and those frames against bank slots.  OpenCV is not available to this build: the rule below
 * is pinned by planted scenes and by a float64 restatement (tests/test_pnp_ransac.py), not against cv2.solvePnPRansac.
 *  - Workspace: fpc_pnp_reserve allocates the pair records (with their mask rows), counts and best keys of max_batch
 *    problems.  It is the only PnP call that allocates or synchronises; the allocation is its own (guard zones under
 *    FPC_PLAN_GUARD_ZONES), freed by fpc_destroy; FPC_E_INVALID when a reservation exists.  It needs no bank and carves
 *    nothing from the ctx slab: the plan hash, the packed size, fpc_bank_get().bytes and the RANSAC pair-list workspace stay
 *    what they are.  `bytes` (may be NULL) gets the size.
 *  - Landmarks: fpc_bank_landmarks_reserve (needs a bank; FPC_E_INVALID when a reservation exists) allocates float4
 *    [slots][rows], zeroed so that no row is valid, with the same guard zones; fpc_bank_destroy and fpc_destroy free it.
 *    fpc_bank_store_landmarks(slot, xyz_dev float32 [rows][3], valid_dev uint8 [rows] or NULL = every row valid): rows
 *    i < count[slot] (read on the device) get (X, Y, Z, valid && all three finite ? 1 : 0), rows behind the count get four
 *    zeros.  Only the first `rows` rows of either array are read, and rows <= capacity, so `xyz + f * cap * 3` and
 *    `front + f * cap` of a fpc_pose_* call go in unchanged, right behind fpc_bank_store(f, slot): the strides are
 *    compatible.  The landmarks are in THAT key frame's camera frame, at the scale the caller gave them.
 *    fpc_bank_landmarks_get returns the storage (float4 [slots][rows], w = 1 valid / 0).  With a reservation alive,
 *    fpc_bank_store, fpc_bank_store_rows and fpc_bank_clear invalidate (zero) the landmarks of the slots they touch with
 *    one more small launch, so that old points never attach to new rows: store the landmarks AFTER the rows.  Without a
 *    reservation those calls do exactly what they did.
 *  - Pairs.  Explicit: pair k < npairs[f] (clamped to [0, stride]) is (xy[f][k], xyz[f][k]); xy_dev float32 [n][stride][2],
 *    xyz_dev float32 [n][stride][3].  Frames and bank: for query row i < count[f] with 0 <= j = match[f][i] < the train
 *    count and landmark j valid, the pair is (xy[f][i], landmark[j]), in ascending i.  For fpc_pnp_frames the landmarks are
 *    key_xyz_dev float32 [nkey][3], nkey_dev[0] clamped to the capacity, and landmark j is valid when key_valid_dev[j] != 0
 *    (NULL: every row) and its three coordinates are finite -- the rule of fpc_bank_store_landmarks.  fpc_pnp_frames knows
 *    FPC_PAIR_KEY only (a predecessor frame has no landmarks), so it has no pairing argument.  A bank slot outside
 *    [0, slots), or a bank without landmark storage, leaves the frame without pairs.  The mask inlier_dev (may be NULL) is
 *    uint8 [n][stride] indexed by the pair (explicit) or [n][capacity] indexed by the query row (frames, bank).
 *  - Convention: X_cam = R X + t with det R = +1, and the pixel of X_cam = (X_c, Y_c, Z_c) is (fx X_c / Z_c + cx,
 *    fy Y_c / Z_c + cy): FROM the landmark frame INTO the query camera.  This is the INVERSE direction of fpc_pose_*'s
 *    X_train = R X_query + t.  R_dev float32 [n][9] row-major, t_dev float32 [n][3].
 *  - Inliers: with (a, b, c) = R X + t in fp64 from the returned fp32 R and t, a pair is an inlier when c > 0 and
 *    (fx a - (x - cx) c)^2 + (fy b - (y - cy) c)^2 < reproj_threshold^2 c^2.  ninliers and the mask are those of the
 *    returned pose.
 *  - Sampling: mix() as above with a budget of 32 draws: r = mix(seed ^ mix((f * 4096 + t) * 32 + k)) % M; the first 6
 *    distinct indices are the sample, in that order; a hypothesis that has not found 6 within its 32 draws is degenerate.
 *  - Minimal solve (6-point DLT), in fp64: image points go to x^ = (x - cx) / fx, y^ = (y - cy) / fy; the six landmarks are
 *    translated to their centroid and scaled to an RMS distance of sqrt(3) (a mean squared distance that is not > 0 or not
 *    finite is degenerate).  The 11 x 12 system has the rows [X Y Z 1 0 0 0 0 -x^X -x^Y -x^Z -x^] and
 *    [0 0 0 0 X Y Z 1 -y^X -y^Y -y^Z -y^] of points 0 .. 4 (rows 2i, 2i + 1) and the first row only of point 5.  It is
 *    reduced by Gaussian elimination with FULL pivoting with the tie rules of the 8-point solve, and the null vector comes
 *    from back-substitution with the last column's unknown set to 1.  A last pivot below 1e-10 of the first, or a
 *    non-finite result, makes the sample degenerate.  P (3 x 4, row-major) is denormalised to the landmarks' own
 *    coordinates: P = Pn [s I, -s m; 0 1], m the centroid and s the scale.
 *  - Scoring: P_px = K P is scaled to max |p| = 1, oriented so that w = p3 . (X, 1) > 0 at the sample's first pair
 *    (evaluated in fp64 before rounding), and rounded to fp32.  Hypothesis t counts the pairs with, in fp32 (fmaf, the
 *    products added in the order X, Y, Z onto the fourth column), w = p3 . (X, 1) > 0 and
 *    (p1 . (X, 1) - x w)^2 + (p2 . (X, 1) - y w)^2 < (thr w)^2.  The raw projective camera is scored, as the raw minimal F
 *    and H are; only the winner is made a pose.  Selection: the largest count; ties go to the lower t.
 *  - Best sample -> pose (fp64): re-derive P = [A | a4] in normalised image coordinates, negated if det A < 0.  A^T A is
 *    diagonalised by the cyclic Jacobi of the fundamental section at N = 3: A^T A = V diag(lambda) V^T.  The frame fails
 *    unless lambda_min > 1e-12 lambda_max.  R = A V diag(lambda^-1/2) V^T, sigma = (sqrt(lambda0) + sqrt(lambda1) +
 *    sqrt(lambda2)) / 3, t = a4 / sigma; both rounded to fp32.
 *  - Refit, `refits` times, one Gauss-Newton step each, in fp64: over the inliers of the current fp32 (R, t), with
 *    X_c = R X + t = (a, b, c), u = a / c, v = b / c: residuals r = (fx (u - x^), fy (v - y^)); left perturbation
 *    X_c <- X_c + omega x X_c + upsilon, unknowns xi = (omega, upsilon), so that the rows of J are
 *        fx [-uv, 1 + u^2, -v, 1/c, 0, -u/c],      fy [-(1 + v^2), uv, u, 0, 1/c, -v/c].
 *    The 21 distinct sums of J^T J and the 6 of J^T r are accumulated in a fixed order (no floating-point atomics).  SIGN:
 *    the step solves (J^T J) xi = -J^T r and is applied as it is: R <- E R, t <- E t + upsilon, with
 *    E = I + A [omega]x + B [omega]x^2, A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2, theta = |omega| (A = 1,
 *    B = 1/2 when theta^2 < 1e-16).  The system is solved by Gaussian elimination with partial pivoting; a pivot not above
 *    1e-14 of the largest diagonal entry of J^T J makes it singular.  R and t are rounded to fp32.  Fewer than 6 inliers, a
 *    singular system or a non-finite result keeps the previous pose and ends the refits.
 *  - Failure: a frame with fewer than 6 pairs, with no non-degenerate sample, with a failed rank test, or with fewer than
 *    min_inliers inliers after the last refit gets nine zeros, three zeros, ninliers = 0 and an all-zero mask.
 *  - Caveat: coplanar landmarks leave the DLT at rank < 11.  A slot whose valid landmarks all lie on one plane fails, just
 *    as an exact-homography scene fails the fundamental calls.  For such slots -- the landmarks of a fpc_pose_homography_*
 *    call are coplanar by construction -- use fpc_ransac_p3p / fpc_p3p_frames / fpc_p3p_bank (next section): the same
 *    arguments, a minimal sample that a plane does not defeat.
 *  - Determinism, execution: as for the fundamental calls.  The three entry points give bit-identical outputs on equal pair
 *    lists, and fpc_pnp_bank is bit-identical to fpc_pnp_frames with that slot's landmarks at the SAME frame index.
 *    Everything but the two reserve calls is asynchronous on the ctx stream: no host synchronisation, no device-to-host
 *    copy, no allocation; every count and slot is read on the device.  fpc_detect, fpc_match_bank, fpc_pnp_bank needs no
 *    host call in between.
 * FPC_E_INVALID (nothing is written): everything the fundamental twins refuse for the arguments they share; no PnP
 * reservation; NULL params, R_dev, t_dev or ninliers_dev; fx or fy not > 0 or a non-finite intrinsic; iterations outside
 * 1 .. 4096; reproj_threshold not > 0 (or not below 1e18); refits outside 0 .. 4; min_inliers < 6.  Landmark calls: no bank,
 * no landmark reservation (store, get), a slot outside [0, slots), a NULL xyz_dev.  fpc_pnp_frames: a NULL key_xyz_dev or
 * nkey_dev. */
typedef struct fpc_pnp_params {
  float fx, fy, cx, cy;      /* query camera, pixels; fx, fy > 0                                                          */
  int iterations;            /* 1 .. 4096                                                                                 */
  float reproj_threshold;    /* px, > 0                                                                                   */
  uint32_t seed;
  int refits;                /* 0 .. 4 Gauss-Newton steps on the inlier set                                               */
  int min_inliers;           /* >= 6                                                                                      */
} fpc_pnp_params;
/* fx = fy = 500, centre (320, 240), 1024 iterations, 3.0 px, seed 0, 4 refits, 12 inliers */
int fpc_default_pnp_params(fpc_pnp_params* params);
int fpc_pnp_reserve(fpc_ctx* ctx, size_t* bytes);
int fpc_bank_landmarks_reserve(fpc_ctx* ctx, size_t* bytes);
int fpc_bank_store_landmarks(fpc_ctx* ctx, int slot, const float* xyz_dev, const uint8_t* valid_dev);
int fpc_bank_landmarks_get(fpc_ctx* ctx, const float** xyzw_dev);
int fpc_ransac_pnp(fpc_ctx* ctx, int n, const float* xy_dev, const float* xyz_dev, const int32_t* npairs_dev, int stride,
                   const fpc_pnp_params* params, float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);
int fpc_pnp_frames(fpc_ctx* ctx, int n, const float* key_xyz_dev, const uint8_t* key_valid_dev, const int32_t* nkey_dev,
                   const int32_t* match_dev, const fpc_pnp_params* params, float* R_dev, float* t_dev,
                   int32_t* ninliers_dev, uint8_t* inlier_dev);
int fpc_pnp_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const fpc_pnp_params* params,
                 float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);

/* --- absolute pose from a minimal sample: P3P + 1, where the landmarks may be coplanar -----------------------------------
 * A second absolute-pose model beside the 6-point DLT above, for what the DLT cannot solve: landmarks on one plane (the
 * xyz / front of a fpc_pose_homography_* call are, by construction) and pair lists too short or too contaminated for samples
 * of six.  A sample is FOUR pairs: three give up to four poses in closed form, the fourth picks one.  fpc_ransac_p3p,
 * fpc_p3p_frames and fpc_p3p_bank take the argument lists of fpc_ransac_pnp, fpc_pnp_frames and fpc_pnp_bank, and
 * everything the section above says of workspace (the fpc_pnp_reserve reservation; nothing else is allocated), landmarks,
 * pairs, the mask's indexing, the convention X_cam = R X + t, the inlier rule of the returned pose, the failure outputs,
 * determinism and execution (asynchronous on the ctx stream, no host call needed between fpc_match_bank and fpc_p3p_bank)
 * holds word for word.  Their R, t go into fpc_match_*_guided_pose, fpc_landmarks_* and fpc_sim3_* as the DLT's do.  What
 * differs, in the order of that section (tests/test_p3p_ransac.py restates it in float64):
 *  - Sampling: the same mix(), key and budget of 32 draws; the first 4 distinct indices are the sample, in that order (they
 *    are the first four of the six the DLT would take).  A frame with fewer than 4 pairs fails.
 *  - Minimal solve, in fp64 without contraction, from the sample's pairs 0, 1, 2 with landmarks X_i and unit bearings
 *    f_i = (x^, y^, 1) / sqrt((x^^2 + y^^2) + 1), x^ = (x - cx) / fx, y^ = (y - cy) / fy.  Every three-term sum below is
 *    (first + second) + third.  With a^2 = |X1 - X2|^2, b^2 = |X0 - X2|^2, c^2 = |X0 - X1|^2 (one of them not > 0: a
 *    coincident pair, degenerate), cos alpha = f1 . f2, cos beta = f0 . f2, cos gamma = f0 . f1, q = (a^2 - c^2) / b^2 and
 *    r = (a^2 + c^2) / b^2, Grunert's quartic in v = s2 / s0 (s_i the depth of point i along f_i) has the coefficients
 *        A4 = (q - 1)^2 - 4 (c^2 / b^2) cos^2 alpha
 *        A3 = 4 [q (1 - q) cos beta - (1 - r) cos alpha cos gamma + 2 (c^2 / b^2) cos^2 alpha cos beta]
 *        A2 = 2 [q^2 - 1 + 2 q^2 cos^2 beta + 2 ((b^2 - c^2) / b^2) cos^2 alpha - 4 r cos alpha cos beta cos gamma
 *                + 2 ((b^2 - a^2) / b^2) cos^2 gamma]
 *        A1 = 4 [-q (1 + q) cos beta + 2 (a^2 / b^2) cos^2 gamma cos beta - (1 - r) cos alpha cos gamma]
 *        A0 = (1 + q)^2 - 4 (a^2 / b^2) cos^2 gamma.
 *    The sample is degenerate unless |A4| > 1e-12 max |A_i| (and that maximum is below 1e300).
 *  - Root finder (Ferrari, no iteration but a fixed number of Newton steps).  b_k = A_k / A4; with v = y - b3 / 4 the quartic
 *    is y^4 + p y^2 + g y + h, p = b2 - 3 b3^2 / 8, g = b1 - b3 b2 / 2 + b3^3 / 8, h = b0 - b3 b1 / 4 + b3^2 b2 / 16
 *    - 3 b3^4 / 256.  Its resolvent cubic is m^3 + c2 m^2 + c1 m + c0 with c2 = p, c1 = p^2 / 4 - h, c0 = -g^2 / 8.  With
 *    P = c1 - c2^2 / 3, Q = 2 c2^3 / 27 - c2 c1 / 3 + c0 and D = Q^2 / 4 + P^3 / 27, its largest real root is m = z - c2 / 3,
 *    z = cbrt(-Q / 2 + sqrt D) + cbrt(-Q / 2 - sqrt D) where D > 0, else z = 2 rho cos(acos(clamp(-Q / (2 rho^3), -1, 1)) / 3)
 *    with rho = sqrt(max(-P / 3, 0)) (z = 0 where rho = 0); m then takes TWO Newton steps on the cubic (a step whose result
 *    is not finite is not taken).  The sample is degenerate unless m > 0.  With s = sqrt(2 m), e = p / 2 + m and
 *    k = g / (2 s) the quartic factors into y^2 - s y + (e + k) and y^2 + s y + (e - k), with the discriminants
 *    dA = 2 m - 4 (e + k) and dB = 2 m - 4 (e - k).  The four CANDIDATES, in this order, are
 *        y0 = (s + sqrt dA) / 2,   y1 = (s - sqrt dA) / 2,   y2 = (-s + sqrt dB) / 2,   y3 = (-s - sqrt dB) / 2;
 *    a candidate whose discriminant is negative does not exist.  v = y - b3 / 4 takes TWO Newton steps on the monic quartic
 *    (Horner form; same rule for a non-finite step).  All four are always walked.
 *  - Candidate -> pose.  v > 0 is required; u = ((q - 1) v^2 - 2 q cos beta v + 1 + q) / (2 (cos gamma - v cos alpha)) must be
 *    > 0 and finite (a vanishing denominator fails here); w = 1 + v^2 - 2 v cos beta > 0; s0 = sqrt(b^2 / w), s1 = u s0,
 *    s2 = v s0; C_i = s_i f_i.  The candidate is kept only if ||C0 - C1|^2 - c^2| <= 2e-6 c^2 and ||C1 - C2|^2 - a^2|
 *    <= 2e-6 a^2 (1e-6 on the lengths; |C0 - C2| = b holds by the choice of s0).  The triad of three points p0, p1, p2 is
 *    x = (p1 - p0) / |p1 - p0|, z = c / |c| with c = (p1 - p0) x (p2 - p0), y = z x x -- the Sim(3) section's, with its test:
 *    degenerate unless |c|^2 > 1e-12 |p1 - p0|^2 |p2 - p0|^2 (collinear points).  R = T_C T_X^T from the triads of
 *    (C0, C1, C2) and (X0, X1, X2), R_ij = x_C,i x_X,j + y_C,i y_X,j + z_C,i z_X,j; t = C0 - R X0.
 *  - Disambiguation by the sample's fourth pair: with (a, b, c) = R X3 + t the candidate is eligible when c > 0 (the first
 *    three points have the depths s_i f_i,z > 0 by u, v > 0) and its error e = (fx (a / c) - (x3 - cx))^2
 *    + (fy (b / c) - (y3 - cy))^2 is finite.  The eligible candidate of smallest e wins; ties go to the lower candidate
 *    index.  A sample without an eligible candidate, or with a non-finite R or t, is degenerate.
 *  - Scoring: P = [R | t] takes the place of the DLT's P: K P scaled to max |p| = 1, oriented at the sample's first pair,
 *    rounded to fp32; the same fp32 count, the same selection (largest count, ties to the lower t).
 *  - Best sample -> pose: the best sample's R, t are derived once more by the same procedure and rounded to fp32 (a
 *    non-finite value fails the frame).  There is no polar step: R is a rotation by construction.
 *  - Refit: the DLT rule's Gauss-Newton step, word for word, except that it stops below 4 inliers, not 6.
 *  - Failure: as above with 4 in the place of 6 and no rank test.
 *  - Caveat: three collinear landmarks, or landmarks that coincide, have no unique pose: such samples are degenerate, and
 *    a slot that holds nothing else fails.  A planar slot is fine.
 *  - Bit-identity: the three entry points give bit-identical outputs on equal pair lists, and fpc_p3p_bank is bit-identical
 *    to fpc_p3p_frames with that slot's landmarks at the SAME frame index.
 * FPC_E_INVALID (nothing is written): everything the PnP twins refuse, except that min_inliers >= 4 is accepted. */
int fpc_ransac_p3p(fpc_ctx* ctx, int n, const float* xy_dev, const float* xyz_dev, const int32_t* npairs_dev, int stride,
                   const fpc_pnp_params* params, float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);
int fpc_p3p_frames(fpc_ctx* ctx, int n, const float* key_xyz_dev, const uint8_t* key_valid_dev, const int32_t* nkey_dev,
                   const int32_t* match_dev, const fpc_pnp_params* params, float* R_dev, float* t_dev,
                   int32_t* ninliers_dev, uint8_t* inlier_dev);
int fpc_p3p_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const fpc_pnp_params* params,
                 float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev);

/* --- relative pose from a minimal sample: the 5-point essential matrix + 1 -----------------------------------------------
 * The calibrated twin of the fundamental calls.  fpc_ransac_fundamental samples eight pairs and solves a linear system that
 * knows nothing of the cameras: on pairs that follow a homography it is degenerate (its caveat above), and its samples of
 * eight ask for 0.4^8 = 6.6e-4 all-inlier draws at 60 % outliers.  Whoever calls fpc_pose_* holds both cameras' intrinsics;
 * with them the relative pose has five degrees of freedom, five pairs determine it (0.4^5 = 1.0e-2; 4.1e-3 with the sixth
 * pair counted), and the five-point problem is NOT degenerate on a plane.  fpc_ransac_essential, fpc_essential_frames and
 * fpc_essential_bank mirror fpc_ransac_fundamental, fpc_fundamental_frames and fpc_fundamental_bank argument for argument
 * -- the same pair definition, mask indexing, strides, pairing, slot rules, workspace (the ctx's pair lists: nothing is
 * allocated), execution rules and determinism -- with fpc_essential_params (the fields of fpc_ransac_params, then the two
 * cameras as in fpc_pose_params) and one more output.  tests/test_essential_ransac.py restates the rule in float64.
 *  - Outputs: F_dev float32 [n][9] IN THE FUNDAMENTAL CALLS' FORM: (u, v, 1) F (x, y, 1)^T = 0 in pixels, Frobenius norm 1,
 *    the element of largest magnitude (of the fp32 values; ties: the lowest index) positive; F = K_t^-T E K_q^-1.  It goes
 *    into fpc_pose_*, fpc_refine_pose_* and the epipolar guided matchers unchanged.  E_dev float32 [n][9], may be NULL: the
 *    same matrix in normalised coordinates, K_t^T F K_q formed in fp64 from the returned fp32 F, norm 1, rounded to fp32,
 *    the same sign rule (so E_dev may be -K_t^T F K_q).  ninliers and inlier are those of the returned fp32 F under the
 *    fundamental section's Sampson test in pixels, in fp64: a later fpc_pose_* call with the same threshold uses exactly
 *    the pairs of this mask.
 *  - Failure: a frame with fewer than 6 pairs, with no non-degenerate sample, or with fewer than min_inliers inliers after
 *    the last refit gets zeros in F_dev and E_dev, ninliers = 0 and an all-zero mask.
 *  - Sampling: the fundamental section's draws (mix(), the key (f * 4096 + t) * 32 + k, 32 draws); the first 6 distinct
 *    indices are the sample, in that order (the first six of the eight the 8-point would take).  Pairs 0 .. 4 are solved,
 *    pair 5 picks the root.
 *  - Minimal solve, in fp64 without contraction (a * b + c is two roundings everywhere).  Bearings p^ = ((x - q_cx) / q_fx,
 *    (y - q_cy) / q_fy, 1), q^ = ((u - t_cx) / t_fx, (v - t_cy) / t_fy, 1).  The 5 x 9 system of the rows q^ (x) p^ =
 *    [ux uy u vx vy v x y 1] is reduced by the 8-point's elimination with FULL pivoting (the same pivot order and tie rule;
 *    a last pivot below 1e-10 of the first: degenerate).  Its free unknowns are those of the columns 5 .. 8 after the
 *    pivoting; setting one of them to 1 and the other three to 0, in that order, and back-substituting (y_i = -(sum_{j > i}
 *    a_ij y_j + a_i,free) / a_ii, the sum in ascending j from 0.0) gives the null vectors X, Y, Z, W, and E = x X + y Y +
 *    z Z + W.
 *  - The ten cubic constraints: det E = 0 and the nine entries, row-major, of (E E^T - tr(E E^T) / 2 I) E = 0, as a 10 x 20
 *    matrix (row 0: det E) over the monomials
 *        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
 *    Every entry of E is a linear polynomial with the coefficients (X, Y, Z, W) over (x, y, z, 1); a product accumulates
 *    into its result from 0.0, one rounded product at a time: linear x linear in the order i, j of the factors'
 *    coefficients, quadratic x linear in the order of the quadratic's monomials (xx xy xz x yy yz y zz z 1), then the
 *    linear factor's; a difference subtracts its second product term by term into the first.  det E = (E11 E22 - E12 E21)
 *    E00 - (E10 E22 - E12 E20) E01 + (E10 E21 - E11 E20) E02, accumulated in that order; (E E^T)_ij = E_i0 E_j0 + E_i1 E_j1
 *    + E_i2 E_j2; tr = ((E E^T)_00 + (E E^T)_11) + (E E^T)_22; row (i, j) = L_i0 E_0j + L_i1 E_1j + L_i2 E_2j with
 *    L = E E^T - tr / 2 I.
 *  - Gauss-Jordan on the left 10 x 10 block with row pivoting: the pivot of column c is the entry of largest magnitude at
 *    or below the diagonal (ties: the lowest row); a pivot not above 1e-12 of the first column's makes the sample
 *    degenerate; the pivot row is divided by the pivot, then a_ic times it is subtracted from every other row i.
 *  - With R the right block, the rows <x^2z> - z <x^2>, <y^2z> - z <y^2>, <xyz> - z <xy> (rows 4 - z 5, 6 - z 7, 8 - z 9)
 *    give B(z) (x, y, 1)^T = 0 with, for the row pair (a, b) and ascending powers of z,
 *        B_x = [Ra2, Ra1 - Rb2, Ra0 - Rb1, -Rb0],  B_y = [Ra5, Ra4 - Rb5, Ra3 - Rb4, -Rb3],
 *        B_1 = [Ra9, Ra8 - Rb9, Ra7 - Rb8, Ra6 - Rb7, -Rb6].
 *    p(z) = det B = B00 (B11 B22 - B12 B21) - B01 (B10 B22 - B12 B20) + B02 (B10 B21 - B11 B20), of degree 10, its products
 *    accumulated as above in the order i, j of the factors' coefficients.
 *  - Real roots, by derivative interlacing with fixed trips.  bound is the first power of two B = 1, 2, 4, .. with
 *    c(B) = |p_10| B^10 - sum_(i < 10) |p_i| B^i > 0 (Cauchy's polynomial by Horner's rule; 64 trips of "B <- 2 B unless
 *    c(B) > 0", then c(B) > 0 or the sample is degenerate): every root lies inside, and it is within a factor 2 of the
 *    best bound of its kind (1 + max |p_i / p_10| is up to 1e14 times wider here).  For d = 1 .. 10, P_d = p^(10 - d) has the coefficients p_(i + 10 - d)
 *    (i + 10 - d)! / i! and the d + 1 break points -bound, the d - 1 values level d - 1 handed on, bound.  Each of its d
 *    intervals [lo, hi], in ascending order, is walked: `change` is (P_d(lo) > 0) != (P_d(hi) > 0); 40 bisections (mid =
 *    (lo + hi) / 2 replaces the end whose sign (P_d > 0) it shares, lo's on a tie of signs); r = (lo + hi) / 2 then takes 3
 *    Newton steps r - P_d(r) / P_d'(r), each kept only where it lies in [lo, hi]; all polynomials by Horner's rule from
 *    the leading coefficient.  The interval hands on r where `change` holds, else its upper end (not a root).  The roots of
 *    p are the values with `change` of level 10, in ascending order.
 *  - Every root z: (x, y, 1) is the null vector of B(z), n = B_row0(z) x B_row1(z), x = n0 / n2, y = n1 / n2 (a non-finite
 *    x or y: no candidate); E = ((x X + y Y) + z Z) + W; F = K_t^-T E K_q^-1.  Choice: the candidate with the smallest
 *    e^2 / g of the sample's sixth pair (e, g the Sampson terms of the fundamental section, in pixels through F, in fp64);
 *    ties go to the lower root.  A sample without a candidate is degenerate, scores 0 and is never chosen.
 *  - Scoring and selection: the candidate's F is scaled to max |f| = 1 and rounded to fp32; the fundamental model's fp32
 *    count and selection (largest count, ties to the lower t).
 *  - The best sample's F, derived once more by the same procedure, brought to norm 1, rounded to fp32 and given the sign.
 *  - Refit, `refits` times, on the essential manifold (the linear 8-point refit would leave it, and has rank 6 on a plane).
 *    The current fp32 F is split by the pose section's decomposition, candidate 0: (R, t^), E = [t^]x R (the twisted pair
 *    gives -E: no cheirality test is needed).  One Gauss-Newton step over the current inliers' Sampson residuals
 *    r = e / sqrt(g) in pixels (e, g through K_t^-T [t^]x R K_q^-1) in the 5 unknowns (omega, eta): R' = Q R with Q the
 *    rotation of the unit quaternion (1, omega / 2) / |(1, omega / 2)| (no trigonometric function is evaluated),
 *    t' = (Q t^ + B eta) / |Q t^ + B eta| with B the refine section's tangent basis of t^.  The Jacobian holds g FIXED:
 *    with a = R p^, dr/d omega = ((t^ x a) x q^) / sqrt(g), dr/d eta_k = (b_k . (a x q^)) / sqrt(g).  The 15 + 5 sums of
 *    J^T J and J^T r are accumulated in fp64 in a fixed order (no floating-point atomics); (J^T J) delta = -J^T r is solved
 *    by elimination with partial pivoting, a pivot not above 1e-14 of the largest diagonal entry failing.  F' = K_t^-T
 *    [t']x R' K_q^-1, norm 1, fp32, sign.  The step is ACCEPTED only if F' has at least as many inliers as F; otherwise,
 *    and with fewer than 6 inliers, a failed decomposition, a singular system, |Q t^ + B eta| <= 1e-12 or a non-finite
 *    result, the previous F stays and the refits end.
 *  - Determinism: as for the fundamental calls; the three entry points give bit-identical outputs on equal pair lists, and
 *    fpc_essential_bank is bit-identical to fpc_essential_frames with that slot as key at the SAME frame index.
 *  - Caveats: a pair list that lies EXACTLY on a plane is explained by two essential matrices (the twofold ambiguity
 *    fpc_pose_homography_* reports as two solutions); no sixth coplanar pair and no count of inliers tells them apart.  The
 *    call returns ONE of them and either is correct output.  Under a pure rotation every [t]x R fits: the call succeeds and t
 *    is meaningless; min_baseline of the homography pose calls is the test for that.
 * FPC_E_INVALID (nothing is written): everything the fundamental twin refuses for the shared fields and fpc_pose_* for the
 * cameras (a focal length not > 0, a non-finite intrinsic), and min_inliers < 6. */
typedef struct fpc_essential_params {
  int      iterations;        /* T hypotheses per frame, 1 .. 4096                                   */
  float    reproj_threshold;  /* pixels (Sampson), > 0                                               */
  uint32_t seed;              /* same seed + same inputs -> bit-identical outputs                    */
  int      refits;            /* 0 .. 4 guarded Gauss-Newton steps after the best sample             */
  int      min_inliers;       /* >= 6; fewer inliers after the last refit -> the frame fails         */
  float    q_fx, q_fy, q_cx, q_cy;   /* the query / src camera                                       */
  float    t_fx, t_fy, t_cx, t_cy;   /* the train / dst camera                                       */
} fpc_essential_params;
/* 1024 iterations, 3.0 px, seed 0, 2 refits, 8 inliers; both cameras (500, 500, 320, 240). */
int fpc_default_essential_params(fpc_essential_params* params);
int fpc_ransac_essential(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                         int stride, const fpc_essential_params* params, float* F_dev, float* E_dev, int32_t* ninliers_dev,
                         uint8_t* inlier_dev);
int fpc_essential_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                         const int32_t* match_dev, const fpc_essential_params* params, float* F_dev, float* E_dev,
                         int32_t* ninliers_dev, uint8_t* inlier_dev);
int fpc_essential_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev,
                       const fpc_essential_params* params, float* F_dev, float* E_dev, int32_t* ninliers_dev,
                       uint8_t* inlier_dev);

/* --- pose-guided matching: the match once more, under the estimated absolute poses as the gate ----------------------------
 * The third model's second pass, "search by projection": with one (R, t) per frame -- what fpc_pnp_frames / fpc_pnp_bank
 * wrote, passed on unchanged, or the previous frame's pose as a motion prior -- the train set's landmarks are projected into
 * the frame and a row is matched only against the landmarks that project next to it.  The gate knows a landmark's depth:
 * two landmarks on one viewing ray of the key camera share their epipolar line, and this gate still tells them apart.
 *
 * fpc_match_frames_guided_pose / fpc_match_bank_guided_pose.  Query sets, counts, cap and the output shapes are
 * fpc_match_frames' for the same n.
 *  - Frames variant: the train set is the key, key_dev float32 [nkey][D] with nkey_dev[0] read on the device and clamped to
 *    the capacity; its landmarks are key_xyz_dev float32 [nkey][3] and key_valid_dev uint8 [nkey] or NULL -- the arguments
 *    and the validity rule of fpc_pnp_frames: landmark j is valid when key_valid_dev[j] != 0 (NULL: every row) and its three
 *    coordinates are finite.  There is no pairing argument and no key_xy_dev: a predecessor frame has no landmarks, and the
 *    gate does not read train pixels.
 *  - Bank variant: frame f's train set is desc[slot[f]], count[slot[f]] of the bank, its landmarks the bank's float4 row
 *    (w != 0: valid).  slot_dev is read on the device; a slot outside [0, slots) gives the frame no train rows.  A bank
 *    without a landmark reservation leaves every row -1 / +inf, as fpc_pnp_bank leaves such a frame without pairs.
 *  - R_dev float32 [n][9] row-major and t_dev float32 [n][3] with X_cam = R X + t: the direction and layout fpc_ransac_pnp /
 *    fpc_pnp_frames / fpc_pnp_bank write.  The camera is four host floats, the fx, fy, cx, cy of fpc_pnp_params.
 *  - Gate: query row i at the integer pixel (x, y), train row j with landmark (X, Y, Z); in fp64 from the fp32 R and t
 *        a = R0 X + R1 Y + R2 Z + t0,   b = R3 X + R4 Y + R5 Z + t1,   c = R6 X + R7 Y + R8 Z + t2
 *        ex = fx a - (x - cx) c,        ey = fy b - (y - cy) c
 *    and row j is a CANDIDATE of row i iff landmark j is valid, c > 0 and ex^2 + ey^2 < radius^2 c^2.  No division.  This
 *    is the inlier test of the PnP calls with radius in the place of reproj_threshold: a pair that a PnP call marks as an
 *    inlier at threshold t is a candidate at radius t.  A failed frame's zeros give c = 0: no candidates, every row
 *    -1 / +inf.  The same holds for an R or t with any non-finite entry.  R is used as given; it is not orthonormalised.
 *  - Result: fpc_match_frames' rule over the candidates only: the nearest candidate in (d^2, index) order, dist = its
 *    distance, max_dist and ratio as there with the second-nearest CANDIDATE as d2 (fewer than two candidates: the ratio
 *    test fails).  Cross check: row i survives iff i is the (d^2, index)-nearest among the query rows that have j as a
 *    candidate.  A row without a candidate: -1 / +inf; rows count[f] <= i < cap: -1 / +inf.
 *  - Bits: for a candidate pair d^2 is the value fpc_match_frames computes for that pair (the same norms, K order,
 *    expression and clamp), so where the guided winner equals the unguided winner dist is bit-equal, and under a radius at
 *    which EVERY pair of a frame is a candidate the frame's output is fpc_match_frames' / the fpc_match_bank table's, bit
 *    for bit.  That needs every train landmark valid with c > 0; the radius that admits every pair depends on the pose.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation (the
 *    workspace is fpc_match_frames', carved at fpc_create; nothing new is carved, the plan hash and the guard zones are what
 *    they were, nothing is added to the bank's or the landmarks' allocation; no fpc_pnp_reserve is needed); every count and
 *    slot is read on the device; deterministic (bit-identical outputs on repeated calls).  fpc_detect, fpc_match_bank,
 *    fpc_pnp_bank, fpc_match_bank_guided_pose, fpc_pnp_bank needs no host call in between; the same holds with a key
 *    through fpc_match_frames, fpc_pnp_frames, fpc_match_frames_guided_pose, fpc_pnp_frames.
 * Non-finite descriptor rows: fpc_match's rule on the fp32 d^2 -- such a pair is no candidate's minimum, no column minimum,
 * no second best, and a row with no candidate at a finite distance is -1 / +inf.
 * FPC_E_INVALID (nothing is written): everything fpc_match_frames refuses; NULL R_dev, t_dev or match_dev; radius not finite
 * or not > 0; fx or fy not > 0 or a non-finite intrinsic; frames variant: NULL key_dev, nkey_dev or key_xyz_dev; bank
 * variant: no bank, NULL slot_dev, or a FPC_BANK_BF16 bank (that format's pose gate is a follow-up, as its epipolar one).
 * The cell-ordered variant is a follow-up too: its train order would have to follow the PROJECTED pixels, which differ per
 * frame and pose. */
int fpc_match_frames_guided_pose(fpc_ctx* ctx, int n, const float* key_dev, const int32_t* nkey_dev,
                                 const float* key_xyz_dev, const uint8_t* key_valid_dev,
                                 const float* R_dev, const float* t_dev, float fx, float fy, float cx, float cy,
                                 float radius, int cross_check, float max_dist, float ratio,
                                 int32_t* match_dev, float* dist_dev);
int fpc_match_bank_guided_pose(fpc_ctx* ctx, int n, const int32_t* slot_dev,
                               const float* R_dev, const float* t_dev, float fx, float fy, float cx, float cy,
                               float radius, int cross_check, float max_dist, float ratio,
                               int32_t* match_dev, float* dist_dev);

/* --- verified relocalisation by pose: the K best slots of the bank per frame, each checked by PnP, P3P, F or E ------------
 * fpc_homography_bank_topk verifies the shortlist of fpc_match_bank_topk with a homography: in a scene with depth that is a
 * pick but not a pose, and the inlier share of a homography on such a scene is arbitrary.  The calls below run the absolute-
 * pose models (fpc_pnp_bank, fpc_p3p_bank) and the epipolar models (fpc_fundamental_bank, fpc_essential_bank) against EVERY
 * candidate, pick the candidate with the most inliers and hand its model on -- without a host loop over the candidates.
 *
 * fpc_pnp_topk_reserve: needs a bank and a fpc_bank_topk_reserve reservation, whose kmax it takes.  The ONLY call of this
 * section that allocates or synchronises: the pair records [max_batch kmax][cap][2] float4, pair counts and best keys of
 * max_batch x kmax absolute-pose problems, in an allocation of its own.  *bytes (may be NULL) receives its size;
 * fpc_bank_get().bytes, the top-K reservation, the PnP reservation and fpc_create's workspace are what they were.  No
 * fpc_pnp_reserve is needed.  FPC_E_INVALID without a bank, without a top-K reservation or when it already exists;
 * fpc_bank_destroy and fpc_destroy free it.  In a FPC_PLAN_GUARD_ZONES context every buffer of it is followed by a canary
 * zone of its own, and fpc_check_guards counts those too.  The epipolar calls run on fpc_bank_topk_reserve's workspace, as
 * fpc_homography_bank_topk does, and need no reservation of this kind.
 *
 * fpc_pnp_bank_topk / fpc_p3p_bank_topk: one absolute-pose problem per (frame, candidate).  1 <= k <= kmax; cand_slot_dev
 * [n][k] and match_dev [n][k][cap] are fpc_match_bank_topk's; R_dev float32 [n][k][9], t_dev float32 [n][k][3], ninliers_dev
 * int32 [n][k], inlier_dev uint8 [n][k][cap] (may be NULL).
 *  - Problem (f, j) is bit-identical to fpc_pnp_bank / fpc_p3p_bank(n, slot = cand_slot[.][j], match = match[.][j], params)
 *    at frame index f -- R, t, ninliers and the mask, failures included: a candidate of -1, a slot outside the bank, a slot
 *    without valid landmarks, a bank without landmark storage and fewer pairs than the sample (6 / 4) each give zeros, 0 and
 *    an all-zero mask.  The sampler and the refit's re-derivation hash f, not f k + j.
 *  - pick_dev int32 [n] (may be NULL): the j with the largest ninliers[f][j], ties to the LOWER j; -1 when every
 *    ninliers[f][.] is 0.  best_dev int32 [n] (may be NULL): cand_slot[f][pick[f]], or -1.  The integer key
 *    (ninliers << 32) | ~j of fpc_homography_bank_topk: independent of the execution order.
 *  - best_R_dev float32 [n][9], best_t_dev float32 [n][3] (both may be NULL): R[f][pick[f]] and t[f][pick[f]], zeros where
 *    pick[f] is -1 -- written on the device, ready for fpc_match_bank_guided_pose(best, best_R, best_t), which leaves a
 *    frame with R = t = 0 without matches, and fpc_pnp_bank(best) behind it.
 *  - A candidate whose landmarks do not belong to the frame's scene collects NO inliers to speak of under an absolute-pose
 *    model (0 of about 640 pairs on the scene of tests/test_pose_bank_topk.py), so min_inliers alone already rejects it.
 * fpc_fundamental_bank_topk / fpc_essential_bank_topk: the same shape on the epipolar models.  F_dev float32 [n][k][9] (and
 * E_dev float32 [n][k][9] of the essential call, may be NULL), ninliers_dev, inlier_dev, pick_dev and best_dev as above;
 * best_F_dev float32 [n][9] (may be NULL): F[f][pick[f]], zeros where pick[f] is -1, ready for
 * fpc_match_bank_guided_epipolar(best, best_F) and fpc_pose_bank.
 *  - Problem (f, j) is bit-identical to fpc_fundamental_bank / fpc_essential_bank with column j, at frame index f.
 *  - Needs keypoints only; nothing is allocated (fpc_bank_topk_reserve's pair lists, rows, counts and best keys).
 *  - WARNING: an epipolar model constrains a pair to a line, not to a point, so a scrambled candidate still collects CHANCE
 *    inliers: 15 - 36 of about 640 pairs at 3 px on the scene above, where the true slot keeps 606 - 613.  min_inliers is
 *    therefore the CALLER's floor against chance, and pick is by maximum, not by the first candidate that passes.
 * Execution: the four calls are asynchronous on the ctx stream, with no host synchronisation, no device-to-host copy and no
 * allocation; counts and slots are read on the device; repeated calls give bit-identical outputs.  The number of launches of
 * a call (gather, score, refit, pick) does not depend on n or k.  fpc_detect, fpc_match_bank_topk, fpc_p3p_bank_topk,
 * fpc_match_bank_guided_pose(best, best_R, best_t), fpc_pnp_bank(best) needs no host call in between.
 * FPC_E_INVALID (nothing is written): everything the single-slot call (fpc_pnp_bank but its fpc_pnp_reserve, fpc_p3p_bank,
 * fpc_fundamental_bank, fpc_essential_bank) refuses; no fpc_bank_topk_reserve; no fpc_pnp_topk_reserve (absolute-pose
 * calls); k outside [1, kmax]; a NULL cand_slot_dev, match_dev, R_dev / t_dev or F_dev, or ninliers_dev. */
int fpc_pnp_topk_reserve(fpc_ctx* ctx, size_t* bytes);
int fpc_pnp_bank_topk(fpc_ctx* ctx, int n, int k, const int32_t* cand_slot_dev, const int32_t* match_dev,
                      const fpc_pnp_params* params, float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev,
                      int32_t* pick_dev, int32_t* best_dev, float* best_R_dev, float* best_t_dev);
int fpc_p3p_bank_topk(fpc_ctx* ctx, int n, int k, const int32_t* cand_slot_dev, const int32_t* match_dev,
                      const fpc_pnp_params* params, float* R_dev, float* t_dev, int32_t* ninliers_dev, uint8_t* inlier_dev,
                      int32_t* pick_dev, int32_t* best_dev, float* best_R_dev, float* best_t_dev);
int fpc_fundamental_bank_topk(fpc_ctx* ctx, int n, int k, const int32_t* cand_slot_dev, const int32_t* match_dev,
                              const fpc_ransac_params* params, float* F_dev, int32_t* ninliers_dev, uint8_t* inlier_dev,
                              int32_t* pick_dev, int32_t* best_dev, float* best_F_dev);
int fpc_essential_bank_topk(fpc_ctx* ctx, int n, int k, const int32_t* cand_slot_dev, const int32_t* match_dev,
                            const fpc_essential_params* params, float* F_dev, float* E_dev, int32_t* ninliers_dev,
                            uint8_t* inlier_dev, int32_t* pick_dev, int32_t* best_dev, float* best_F_dev);

/* --- map growth: landmarks for a new key frame from its PnP pose ----------------------------------------------------------
 * fpc_pose_* is the only call above that creates 3-D points, from two views and at the scale |t| = 1 of that pair.  A frame
 * that fpc_pnp_frames / fpc_pnp_bank has localised has an R, t at the MAP's scale; the calls below give that frame its own
 * landmarks at that scale, so that it can be stored as the next key frame: a row that matched a train row WITH a landmark
 * gets that landmark carried over into its own camera frame, a row that matched a train row WITHOUT one gets a new point,
 * triangulated under the known pose.  fpc_landmarks_pairs, fpc_landmarks_frames and fpc_landmarks_bank mirror
 * fpc_ransac_pnp, fpc_pnp_frames and fpc_pnp_bank: explicit pairs, the frames of the last detect against one key set, and
 * those frames against bank slots.
 *  - Convention: X_query = R X_train + t, the direction the PnP calls write; R_dev float32 [n][9] row-major and t_dev float32
 *    [n][3] are passed on unchanged.  An R, t from fpc_pose_* has the OPPOSITE direction (X_train = R X_query + t) and does
 *    not go in as it is.  R is used as given; it is not orthonormalised.
 *  - Rows.  Explicit: pair k < npairs[f] (clamped to [0, stride]) is the query pixel q_xy[f][k], the train pixel t_xy[f][k]
 *    (both float32 [n][stride][2]) and the train row's landmark t_xyz[f][k] (float32 [n][stride][3]) with its flag
 *    t_valid[f][k] (uint8 [n][stride]; NULL: every row).  Frames and bank: query row i < count[f] with
 *    0 <= j = match[f][i] < the train count; the query pixel is xy[f][i] of the results, the train pixel and landmark are row
 *    j of the key (key_xy_dev int32 [nkey][2], key_xyz_dev float32 [nkey][3], key_valid_dev uint8 [nkey] or NULL; nkey_dev[0]
 *    clamped to the capacity) or of bank slot slot[f].  Counts, clamping, the slot rules and the key rules are those of
 *    fpc_pnp_frames / fpc_pnp_bank.  A landmark is valid by the rule of fpc_bank_store_landmarks: its flag is set and its
 *    three coordinates are finite.  A NULL t_xyz_dev / key_xyz_dev, or a bank without a landmark reservation, means that no
 *    train row has a landmark.  Everything below is fp64, computed from the fp32 R, t and from integer or fp32 pixels.
 *  - Failed pose: a frame whose R is all zero (a failed frame of the PnP calls), or whose R or t holds a non-finite entry,
 *    and a bank slot outside [0, slots): every kind row 0, every xyz row zero, counts (0, 0).
 *  - Transfer (kind 1), where the train row has a valid landmark X: (a, b, c) = R X + t; the row is kept iff c > 0 and
 *        (q_fx a - (x - q_cx) c)^2 + (q_fy b - (y - q_cy) c)^2 < reproj_threshold^2 c^2
 *    with (x, y) the query pixel: the inlier test of the PnP calls.  xyz = (a, b, c) rounded to fp32.  A row that fails gets
 *    kind 0; it is NOT triangulated: the map contradicts the match.
 *  - Triangulation (kind 2), where the train row has no valid landmark: p^ = ((x - q_cx) / q_fx, (y - q_cy) / q_fy, 1), q^
 *    likewise from the train pixel (u, v) and the train camera; a = p^, b = R q^;
 *        det = (a.a)(b.b) - (a.b)^2,
 *        lam = ((a.t)(b.b) - (a.b)(b.t)) / det,      mu = ((a.b)(a.t) - (a.a)(b.t)) / det
 *    (the parameters at which the rays lam a and t + mu b are closest); X = (lam a + t + mu b) / 2, the midpoint, in the query
 *    camera's frame, and Y = R^T (X - t), the same point in the train camera's frame.  The row is kept iff
 *        det > sin^2(min_parallax_deg) (a.a)(b.b)   (sin^2 formed by the host in double; at 0 degrees the floor of the pose
 *                                                     calls instead: det > 1e-12 (a.a)(b.b)),
 *        lam > 0 and mu > 0,
 *        X passes the test above against the query pixel and the query camera,
 *        Y passes it against the train pixel and the train camera,
 *    all of them on the fp64 X, before rounding.  xyz = X rounded to fp32.
 *  - Outputs: xyz_dev float32 [n][S][3], kind_dev uint8 [n][S], counts_dev int32 [n][2] (may be NULL); S is `stride` for
 *    fpc_landmarks_pairs and the capacity for the other two; a row is a pair (explicit) or a query row (frames, bank).  Every
 *    row of the call's frames is written: nothing needs to be cleared beforehand.  A row that is no pair, lies past the
 *    count or failed a test holds kind 0 and three zeros.  counts[f] = (rows of kind 1, rows of kind 2): integer sums,
 *    independent of the execution order.  kind_dev + f S goes into fpc_bank_store_landmarks as valid_dev unchanged (it tests
 *    != 0) and xyz_dev + f S 3 as xyz_dev, right behind fpc_bank_store(f, slot): fpc_detect, fpc_match_bank, fpc_pnp_bank,
 *    fpc_landmarks_bank, fpc_bank_store, fpc_bank_store_landmarks needs no host call in between, and the map grows at one
 *    scale.
 *  - Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation.  One launch
 *    reads every row straight from its source: nothing is carved, the RANSAC and PnP pair-list workspaces are not touched, so
 *    no fpc_pnp_reserve is needed; the plan hash and the guard zones are what they were.  Every count and slot is read on the
 *    device.  Deterministic: bit-identical outputs on repeated calls; the three entry points give bit-identical outputs on
 *    equal lists, and fpc_landmarks_bank is bit-identical to fpc_landmarks_frames with that slot's own storage as the key.
 *    It works on a FPC_BANK_BF16 bank: it reads only xy, counts and landmarks.
 *  - Not here: fusing repeated observations of one landmark, bundle adjustment over more than two views, a cell-ordered
 *    variant.
 * FPC_E_INVALID (nothing is written): everything the PnP twins refuse for the arguments they share (n, stride, a NULL pair
 * array, npairs_dev, match_dev); NULL params, R_dev, t_dev, xyz_dev or kind_dev; fx or fy not > 0 or a non-finite intrinsic on
 * either side; reproj_threshold not > 0 (or not below 1e18); min_parallax_deg not in [0, 90); fpc_landmarks_frames: a NULL
 * key_xy_dev or nkey_dev; fpc_landmarks_bank: no bank or a NULL slot_dev. */
typedef struct fpc_landmark_params {
  float q_fx, q_fy, q_cx, q_cy;   /* camera of the frames being promoted (query), pixels, fx, fy > 0                      */
  float t_fx, t_fy, t_cx, t_cy;   /* camera of the key frame (train)                                                      */
  float reproj_threshold;         /* px, > 0, below 1e18                                                                  */
  float min_parallax_deg;         /* >= 0, < 90: the least angle between the two rays of a triangulated row               */
} fpc_landmark_params;
/* fx = fy = 500, centre (320, 240) on both sides, reproj_threshold 3.0, min_parallax_deg 1.0 */
int fpc_default_landmark_params(fpc_landmark_params* params);
int fpc_landmarks_pairs(fpc_ctx* ctx, int n, const float* q_xy_dev, const float* t_xy_dev, const float* t_xyz_dev,
                        const uint8_t* t_valid_dev, const int32_t* npairs_dev, int stride, const float* R_dev,
                        const float* t_dev, const fpc_landmark_params* params, float* xyz_dev, uint8_t* kind_dev,
                        int32_t* counts_dev);
int fpc_landmarks_frames(fpc_ctx* ctx, int n, const int32_t* key_xy_dev, const int32_t* nkey_dev, const float* key_xyz_dev,
                         const uint8_t* key_valid_dev, const int32_t* match_dev, const float* R_dev, const float* t_dev,
                         const fpc_landmark_params* params, float* xyz_dev, uint8_t* kind_dev, int32_t* counts_dev);
int fpc_landmarks_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const float* R_dev,
                       const float* t_dev, const fpc_landmark_params* params, float* xyz_dev, uint8_t* kind_dev,
                       int32_t* counts_dev);

/* --- two-view bundle adjustment: refine R, t and the points of a pose call --------------------------------------------------
 * fpc_pose_* and fpc_pose_homography_* are linear: R and t come from decomposing an F or an H that RANSAC fitted
 * algebraically, and every point is the midpoint of two rays.  fpc_refine_pose, fpc_refine_pose_frames and
 * fpc_refine_pose_bank minimise what a mapper cares about -- the reprojection error in both images -- over R, the direction
 * of t and one point per pair, by damped Gauss-Newton steps (Levenberg-Marquardt) on the device.  They mirror
 * fpc_pose_fundamental / fpc_pose_frames / fpc_pose_bank argument for argument: the same pair definition, strides, clamping
 * of counts, pairing, key and slot rules and pair-list workspace, with the input pose R_in_dev float32 [n][9] row-major and
 * t_in_dev float32 [n][3] in the place of F_dev and fpc_refine_params in the place of fpc_pose_params.  What fpc_pose_* wrote
 * goes in unchanged; one solution of fpc_pose_homography_* goes in once its [n][2] slice has been made contiguous.
 * Outputs: R_dev, t_dev, nfront_dev and front_dev (may be NULL) as for fpc_pose_*; xyz_dev float32 [n][S][3] is REQUIRED: it
 * is the state of the iteration; stats_dev float32 [n][4] (may be NULL): the rms reprojection error over the members before,
 * the same after, attempts made, attempts accepted.  R_dev / t_dev may alias R_in_dev / t_in_dev.  Everything below is fp64
 * unless said otherwise.
 *  - Convention: X_train = R X_query + t, |t| = 1, the points in the query camera's frame at that scale: the pose calls'.
 *  - Input: a frame fails if R_in is all zero (a failed frame of the pose calls), if R_in or t_in holds a non-finite entry, or
 *    if |t_in| is not > 0.  Otherwise R = R_in and t = t_in / |t_in| rounded to fp32.  R is used as given; it is not
 *    orthonormalised.
 *  - Members: every pair of the list is triangulated under (R, t) exactly as in the pose section (a = R p^, b = q^, det, lam,
 *    mu); X = (lam p^ + R^T (mu q^ - t)) / 2 is the midpoint.  A pair is a MEMBER iff
 *        det > sin^2(min_parallax_deg) (a.a)(b.b)   (sin^2 formed by the host in double; at 0 degrees, and wherever sin^2 is
 *                                                     below it, the floor of the pose calls: det > 1e-12 (a.a)(b.b)),
 *        lam > 0 and mu > 0,
 *        X passes the reprojection test of the landmark section against the query pixel and the query camera,
 *        R X + t passes it against the train pixel and the train camera,
 *    and X rounded to fp32, the start point, has a third coordinate > 0.  The membership is fixed for the whole call.
 *  - Cost: C = sum over the members of |pi_q(X) - p|^2 + |pi_t(R X + t) - q|^2 with pi(Y) = (fx Y0 / Y2 + cx, fy Y1 / Y2 + cy),
 *    p the query pixel and q the train pixel, evaluated from the fp32 state (R, t, X).  A state with a member whose depth
 *    (X2, or the third coordinate of R X + t) is not > 0 has C = +inf.
 *  - Unknowns and gauge: dX (three) per member; for the train camera the left perturbation of the PnP refit,
 *    X_c <- X_c + omega x X_c + upsilon with X_c = R X + t; the query camera is the origin.  The scale is fixed by
 *    upsilon = B eta, B = [b1 b2] orthogonal to t: with k the index of the smallest |t_k| (ties to the lowest index),
 *    b1 = (t x e_k) / |t x e_k| and b2 = (t x b1) / |t x b1|.  That leaves 5 pose unknowns delta = (omega, eta).
 *  - Per member, with J_p(Y) = [fx / Y2, 0, -fx Y0 / Y2^2; 0, fy / Y2, -fy Y1 / Y2^2] and the residuals r_q = pi_q(X) - p,
 *    r_t = pi_t(X_c) - q:
 *        J_q = J_p(X) (query camera),   J_t = J_p(X_c) R,   J_c = [-J_p(X_c) [X_c]x , J_p(X_c) B]   (2 x 5),
 *        U = J_q^T J_q + J_t^T J_t,     W = J_c^T J_t   (5 x 3),     g_X = J_q^T r_q + J_t^T r_t.
 *  - Damping (Marquardt): U* = U + lambda diag(U); its inverse is the adjugate over the determinant, and a determinant that
 *    is not > 0 or not finite (at any member) rejects the attempt.  With A = sum J_c^T J_c and g_c = sum J_c^T r_t:
 *        S = A + lambda diag(A) - sum W U*^-1 W^T,        b = g_c - sum W U*^-1 g_X:
 *    15 + 5 + 5 sums (S without its damping, diag A, b), accumulated per thread over a fixed stride and summed in a fixed
 *    order (no floating-point atomics).
 *  - Step: S delta = -b by Gaussian elimination with partial pivoting; a pivot not above 1e-14 of the largest diagonal entry
 *    of S makes it singular and rejects the attempt.  R' = E(omega) R with E as in the PnP refit; t' = E t + B eta;
 *    s = 1 / |t'| and t' <- s t' (|t'| not > 1e-12 rejects the attempt); dX = -U*^-1 (g_X + W^T delta) and X' = s (X + dX).
 *    R', t' and X' are rounded to fp32 and C' is evaluated from them.
 *  - Accept and reject: the step is accepted iff C' < C; then lambda <- max(lambda / 10, 1e-10).  Otherwise the state is kept
 *    and lambda <- min(10 lambda, 1e6).  Either way it counts as one attempt.  lambda starts at lambda0.  The call ends after
 *    `iterations` attempts, or after an accepted step with C - C' <= 1e-6 C.
 *  - Result: front[row] = 1 for the members that, at the final state, have a depth > 0 in both cameras and pass both
 *    reprojection tests; xyz[row] holds their points; every other row of the frame is zero; nfront is their count.  The rms
 *    of stats is sqrt(C / (2 m)) over the m members -- the root mean square of the 2 m reprojection distances -- at the start
 *    and at the final state.  The outputs never have a higher cost than the input state: a frame on which no attempt was
 *    accepted returns the input pose (t normalised) with its midpoints.  The call writes every row of its frames' front /
 *    xyz: nothing needs to be cleared beforehand.
 *  - Failure: a failed input, no pairs, or nfront < min_front: nine zeros, three zeros, nfront = 0, an all-zero front and
 *    xyz, four zero stats.  A bank slot outside [0, slots) leaves the frame without pairs and fails the same way.
 *  - Determinism and execution: as for the pose calls.  Bit-identical outputs on repeated calls; the three entry points give
 *    bit-identical outputs on equal pair lists, and fpc_refine_pose_bank is bit-identical to fpc_refine_pose_frames with that
 *    slot as key.  Asynchronous on the ctx stream, no host synchronisation, no device-to-host copy, no allocation; the point
 *    state lives in the caller's xyz.  Nothing is carved; the plan hash and the guard zones are what they were.
 *    fpc_match_bank, fpc_fundamental_bank, fpc_pose_bank, fpc_refine_pose_bank, fpc_bank_store, fpc_bank_store_landmarks needs
 *    no host call in between.  It works on a FPC_BANK_BF16 bank: it reads only xy and counts.
 *  - Not here: more than two views (fpc_refine_window_* below), robust kernels, refining the intrinsics, a cell-ordered
 *    variant.
 * FPC_E_INVALID (nothing is written): everything the pose twins refuse for the arguments they share; a NULL R_in_dev /
 * t_in_dev / params / R_dev / t_dev / nfront_dev / xyz_dev; fx or fy not > 0 or any non-finite intrinsic; reproj_threshold
 * not > 0 (or not below 1e18); min_parallax_deg not in [0, 90); iterations outside 1 .. 16; lambda0 not > 0 or not finite;
 * min_front < 1. */
typedef struct fpc_refine_params {
  float q_fx, q_fy, q_cx, q_cy;   /* intrinsics of the query camera (pixels), fx, fy > 0                                  */
  float t_fx, t_fy, t_cx, t_cy;   /* intrinsics of the train camera                                                       */
  float reproj_threshold;         /* px, > 0, below 1e18: membership and the final front test                             */
  float min_parallax_deg;         /* >= 0, < 90: as fpc_landmark_params                                                   */
  int   iterations;               /* 1 .. 16 attempts                                                                     */
  float lambda0;                  /* > 0, finite: the first damping                                                       */
  int   min_front;                /* >= 1; fewer points in front at the final state -> the frame fails                    */
} fpc_refine_params;
/* fx = fy = 500, centre (320, 240) on both sides, reproj_threshold 3.0, min_parallax_deg 1.0, iterations 8, lambda0 1e-3,
 * min_front 8 */
int fpc_default_refine_params(fpc_refine_params* params);
int fpc_refine_pose(fpc_ctx* ctx, int n, const float* src_xy_dev, const float* dst_xy_dev, const int32_t* npairs_dev,
                    int stride, const float* R_in_dev, const float* t_in_dev, const fpc_refine_params* params, float* R_dev,
                    float* t_dev, int32_t* nfront_dev, float* xyz_dev, uint8_t* front_dev, float* stats_dev);
int fpc_refine_pose_frames(fpc_ctx* ctx, int n, int pairing, const int32_t* key_xy_dev, const int32_t* nkey_dev,
                           const int32_t* match_dev, const float* R_in_dev, const float* t_in_dev,
                           const fpc_refine_params* params, float* R_dev, float* t_dev, int32_t* nfront_dev, float* xyz_dev,
                           uint8_t* front_dev, float* stats_dev);
int fpc_refine_pose_bank(fpc_ctx* ctx, int n, const int32_t* slot_dev, const int32_t* match_dev, const float* R_in_dev,
                         const float* t_in_dev, const fpc_refine_params* params, float* R_dev, float* t_dev,
                         int32_t* nfront_dev, float* xyz_dev, uint8_t* front_dev, float* stats_dev);

/* --- local bundle adjustment: refine a key frame's landmarks over the frames that see them ---------------------------------
 * Every landmark above comes from two views, and every pose against the map from one view with the landmarks held fixed.
 * fpc_refine_window, fpc_refine_window_frames and fpc_refine_window_bank refine ONE key frame's landmarks and the poses of
 * up to FPC_WINDOW_MAX_FRAMES frames that observe them, together, by damped Gauss-Newton steps (Levenberg-Marquardt) on the
 * reprojection error in all views.  The inputs are what fpc_match_bank + fpc_pnp_bank leave on the device -- a match table
 * per frame against the key and R, t per frame at the map's scale -- and xyz_dev, kind_dev go back into
 * fpc_bank_store_landmarks(slot, xyz_dev, kind_dev) as they are: the chain improves its own map without a host call.
 *  - Window: n frames of the last results, 1 <= n <= min(max_batch, FPC_WINDOW_MAX_FRAMES): the reduced system is at most
 *    96 x 96 in fp64 and is solved in LDS.
 *  - Landmarks: in the key camera's frame, as fpc_bank_store_landmarks defines them; valid by its rule (the flag is set and the
 *    three coordinates are finite).  Explicit: key_xy_dev float32 [P][2], key_xyz_dev float32 [P][3], key_valid_dev uint8 [P]
 *    or NULL, nkey_dev[0] (clamped to the capacity) <= P.  Frames: the key arguments of fpc_landmarks_frames.  Bank: slot
 *    key_slot_dev[0], read on the device; a slot outside [0, slots) or a bank without landmark storage leaves the key without
 *    rows, and the call fails as below.
 *  - Poses: PnP's convention, Y = R_f X + t_f maps into frame f's camera; what fpc_pnp_* / fpc_p3p_* wrote goes in unchanged.
 *  - Observations of frame f.  Frames and bank: query row i < count[f] with 0 <= j = match[f][i] < nkey and landmark j valid,
 *    in ascending i; the pixel is xy[f][i] of the results.  Explicit: pair k < nobs_in[f] (clamped to [0, stride]) with
 *    j = idx[f][k] and the pixel xy[f][k].  When several rows of one frame name the same j, the LOWEST one that passes the
 *    member test is the observation (an integer minimum per (frame, landmark): independent of the execution order).
 *    Bank: frame f takes part iff slot_dev is NULL or slot_dev[f] == key_slot_dev[0] -- fpc_match_bank's table of a frame is
 *    against best[f], so a frame whose best is another slot stays out.
 * The rule.  Everything is fp64 unless said otherwise.
 *  - Live frames: a frame is dead if R_in is all zero, if R_in or t_in holds a non-finite entry, or if the bank variant's
 *    slot test fails.  R is used as given; it is not orthonormalised.  The state is the fp32 inputs.
 *  - Membership, fixed for the whole call and decided in one pass: landmark j is ELIGIBLE iff it is valid and passes the PnP
 *    inlier test of the PnP section (c > 0, division-free) against its own key pixel under the key camera (t_*) with the
 *    identity pose.  An observation is a MEMBER iff its frame is live, its landmark is eligible, R_f X_j + t_f passes that
 *    test against the frame's pixel under the query camera (q_*), and it is the lowest such row of (f, j).  A live frame with
 *    fewer than min_obs members is dropped and its observations stop being members; the others are KEPT.  A landmark is
 *    ACTIVE iff it is eligible and at least one member observation is left.  If no frame is kept the call FAILS: every R, t
 *    and nobs is zero, the stats are zero, the mask is zero and every valid landmark is copied out with kind 2 -- a failed
 *    call never erases a map.
 *  - Cost: C = sum over the active landmarks of |pi_key(X_j) - k_j|^2 + sum over the members of |pi_q(R_f X_j + t_f) - p|^2,
 *    evaluated from the fp32 state; +inf where any depth is not > 0.  rms = sqrt(C / (members + active)).  A landmark's terms
 *    are added key first, then its frames in ascending order; the landmarks of a chunk of 64 key rows in ascending order; the
 *    chunks in ascending order.
 *  - Unknowns: dX (three) per active landmark; per kept frame the six of the PnP refit's left perturbation (omega, upsilon);
 *    the key camera is the origin.  The reduced system has D = 6 x (kept frames) <= 96 unknowns, in ascending frame order.
 *  - Per observation, with Y = R_f X + t_f and J_p as in the refine section: J_X = J_p(Y) R_f, J_c = [-J_p(Y) [Y]x, J_p(Y)]
 *    (2 x 6), r = pi_q(Y) - p.  Per landmark: U_j = J_k^T J_k + sum_f J_X^T J_X and g_j = J_k^T r_k + sum_f J_X^T r (key
 *    first, then the frames in ascending order) with J_k = J_p(X_j) under the key camera and r_k = pi_key(X_j) - k_j;
 *    W_fj = J_c^T J_X (6 x 3).  Per frame: A_f = sum J_c^T J_c, g_f = sum J_c^T r.
 *  - Damping and reduction, as in the refine section: U* = U + lambda diag U, inverted as adjugate over determinant; a
 *    determinant that is not > 0 or not finite, at any landmark, rejects the attempt.
 *        S = A + lambda diag A - sum_j W_j U*^-1 W_j^T,      b = g_c - sum_j W_j U*^-1 g_j
 *    with W_j the stack of the blocks of the frames that observe j.  Order of the sums: every entry of S (A without its
 *    damping folded in per landmark: J_c^T J_c - Y W^T on the diagonal blocks, 0 - Y W^T elsewhere, Y = W U*^-1), of diag A and
 *    of b is accumulated over the landmarks of a chunk of 64 key rows in ascending order, and the chunks' partial sums are
 *    added in ascending order.  There are no floating-point atomics.
 *  - Solve: S delta = -b by Gaussian elimination with partial pivoting (the first largest pivot); a pivot not above 1e-14 of
 *    the largest diagonal entry of S rejects the attempt.  The gauge's null direction is left to the damping.
 *  - Step: R_f' = E(omega_f) R_f and t_f' = E t_f + upsilon_f with E as in the PnP refit; X_j' = X_j - U*^-1 (g_j + sum_f
 *    W_fj^T delta_f), the frames in ascending order.  SCALE GAUGE: with Z0 the sum, in ascending j, of the active landmarks'
 *    third coordinates at the START state, s = Z0 / sum_j X_j'[2] (ascending j); s not finite or not > 0 rejects the attempt;
 *    every t_f' and X_j' is multiplied by s (the cost is invariant under that scaling; fixing the scale by one frame's |t|
 *    instead hands that frame's scale error to the points).  The state is then rounded to fp32 and C' is evaluated from it.
 *  - Accept, reject, stop: exactly the refine section's rule -- accepted iff C' < C, then lambda <- max(lambda / 10, 1e-10);
 *    otherwise the state is kept and lambda <- min(10 lambda, 1e6).  The call stops after `iterations` attempts, or after an
 *    accepted step with C - C' <= 1e-6 C.
 *  - Result: kept frames get their state, dropped and dead frames zeros.  An active landmark that passes the key-pixel test at
 *    the final state gets kind 1; one that fails it gets kind 0 and zeros (culled); a valid landmark that is not active gets
 *    kind 2 and is copied unchanged; everything else, and every row at or beyond nkey, is kind 0 with zeros.  nobs[f]: the
 *    kept frame's member observations whose landmark has kind 1 and that pass the frame's reprojection test at the final
 *    state; obs marks them.  The outputs never cost more than the inputs: a call without an accepted attempt returns the
 *    inputs.  The three entry points give bit-identical outputs on equal observation lists.
 * Outputs: xyz_dev float32 [capacity][3] and kind_dev uint8 [capacity], by key row, are REQUIRED: xyz_dev is the state of the
 * iteration.  R_dev float32 [n][9] and t_dev float32 [n][3] may alias the inputs.  nobs_dev int32 [n].  obs_dev uint8
 * [n][capacity] by query row, or [n][stride] by pair for the explicit variant (may be NULL).  stats_dev float32 [4] (may be
 * NULL): rms before, rms after, attempts made, attempts accepted.  Every row of every output is written.
 * fpc_window_reserve is the only call here that allocates or synchronises: the observation table, the partial sums and the
 * pose state, in an allocation of its own, with guard zones under FPC_PLAN_GUARD_ZONES, freed by fpc_destroy; a second
 * reserve is FPC_E_INVALID.  It carves nothing: the plan hash, the packed size and fpc_bank_get().bytes stay what they are.
 * Execution: asynchronous on the ctx stream, no host synchronisation, no device-to-host copy; every count and slot is read
 * on the device; a fixed sequence of launches per attempt, `iterations` times, which a device flag turns into no-ops once the
 * call has stopped (no cooperative launch, no workgroup waits on another).  Repeated calls give bit-identical outputs.  It
 * works on a FPC_BANK_BF16 bank: it reads xy, counts and landmarks only.  fpc_detect, fpc_match_bank, fpc_pnp_bank,
 * fpc_refine_window_bank, fpc_bank_store_landmarks needs no host call in between.
 *  - Not here: robust kernels, refining the intrinsics, larger windows (more than 16 frames), several key frames' landmarks
 *    in one problem.
 * FPC_E_INVALID (nothing is written): no fpc_window_reserve; what the refine twins refuse for the arguments they share (n,
 * stride, a NULL observation array, match_dev, no bank); n > FPC_WINDOW_MAX_FRAMES; a NULL key_xy_dev, key_xyz_dev, nkey_dev,
 * key_slot_dev, R_in_dev, t_in_dev, params, R_dev, t_dev, nobs_dev, xyz_dev or kind_dev; fx or fy not > 0 or any non-finite
 * intrinsic; reproj_threshold not > 0 (or not below 1e18); iterations outside 1 .. 16; lambda0 not > 0 or not finite;
 * min_obs < 3. */
#define FPC_WINDOW_MAX_FRAMES 16
typedef struct fpc_window_params {
  float q_fx, q_fy, q_cx, q_cy;   /* camera of the n frames (pixels), fx, fy > 0                                          */
  float t_fx, t_fy, t_cx, t_cy;   /* camera of the key frame                                                              */
  float reproj_threshold;         /* px, > 0, below 1e18: membership and the final tests                                  */
  int   iterations;               /* 1 .. 16 attempts                                                                     */
  float lambda0;                  /* > 0, finite: the first damping                                                       */
  int   min_obs;                  /* >= 3: fewer member observations drop a frame                                         */
} fpc_window_params;
/* fx = fy = 500, centre (320, 240) on both sides, reproj_threshold 3.0, iterations 8, lambda0 1e-3, min_obs 6 */
int fpc_default_window_params(fpc_window_params* params);
int fpc_window_reserve(fpc_ctx* ctx, size_t* bytes);
int fpc_refine_window(fpc_ctx* ctx, int n, const float* xy_dev, const int32_t* idx_dev, const int32_t* nobs_in_dev, int stride,
                      const float* key_xy_dev, const float* key_xyz_dev, const uint8_t* key_valid_dev, const int32_t* nkey_dev,
                      const float* R_in_dev, const float* t_in_dev, const fpc_window_params* params, float* R_dev,
                      float* t_dev, int32_t* nobs_dev, float* xyz_dev, uint8_t* kind_dev, uint8_t* obs_dev, float* stats_dev);
int fpc_refine_window_frames(fpc_ctx* ctx, int n, const int32_t* key_xy_dev, const int32_t* nkey_dev, const float* key_xyz_dev,
                             const uint8_t* key_valid_dev, const int32_t* match_dev, const float* R_in_dev,
                             const float* t_in_dev, const fpc_window_params* params, float* R_dev, float* t_dev,
                             int32_t* nobs_dev, float* xyz_dev, uint8_t* kind_dev, uint8_t* obs_dev, float* stats_dev);
int fpc_refine_window_bank(fpc_ctx* ctx, int n, const int32_t* key_slot_dev, const int32_t* slot_dev, const int32_t* match_dev,
                           const float* R_in_dev, const float* t_in_dev, const fpc_window_params* params, float* R_dev,
                           float* t_dev, int32_t* nobs_dev, float* xyz_dev, uint8_t* kind_dev, uint8_t* obs_dev,
                           float* stats_dev);

/* --- Sim(3) alignment: RANSAC similarity between two frames' landmarks ----------------------------------------------------
 * Every key frame carries landmarks in its own camera frame, at the scale it inherited from the key frame it was localised
 * against.  A frame that HAS landmarks of its own (what fpc_landmarks_* wrote) and matches an old bank slot -- a loop
 * candidate of fpc_match_bank_topk -- has 3-D <-> 3-D pairs, and the similarity between the two sets is the edge a pose graph
 * or a map merge needs: R and t as fpc_pnp_bank gives them, and the ratio s of the two scales, the drift a monocular map
 * accumulates (Horn 1987, scored by reprojection in both cameras).  fpc_ransac_sim3, fpc_sim3_frames and fpc_sim3_bank mirror
 * fpc_ransac_pnp, fpc_pnp_frames and fpc_pnp_bank: explicit pairs, the frames of the last detect against one key set, and
 * those frames against bank slots.  The rule below is pinned by planted scenes and by a float64 restatement
 * (tests/test_sim3_ransac.py).
 *  - Convention: X_query = s R X_train + t with det R = +1 and s > 0: the direction the PnP calls write, with the scale
 *    added.  s_dev float32 [n], R_dev float32 [n][9] row-major, t_dev float32 [n][3].  With both sets at one scale this is the
 *    PnP pose; with the train set stored at 1 / sigma of the query's scale it is (sigma, R, sigma t_pnp).
 *  - Pairs.  Explicit: pair k < npairs[f] (clamped to [0, stride]) is (q_xyz[f][k], t_xyz[f][k]), both float32
 *    [n][stride][3].  A pair with a non-finite coordinate on either side is still a pair, a record like any other; it can
 *    never be an inlier (below).  Frames and bank: query row i < count[f] with 0 <= j = match[f][i] < the train count.
 *    q_xyz_dev is float32 [n][capacity][3] and q_valid_dev uint8 [n][capacity] or NULL (every row): the xyz_dev and kind_dev of
 *    a fpc_landmarks_* call, unchanged.  The train landmarks are the key's (key_xyz_dev float32 [nkey][3], key_valid_dev uint8
 *    [nkey] or NULL, nkey_dev[0] clamped to the capacity) or bank slot slot[f]'s float4 rows.  The row is a pair iff BOTH
 *    landmarks are valid by the rule of fpc_bank_store_landmarks: the flag is != 0 and the three coordinates are finite.
 *    Pairs come in ascending i.  The slot rules, the clamping, a bank without a landmark reservation (no frame has pairs) and
 *    the mask's indexing (uint8 [n][stride] by pair, or [n][capacity] by query row; may be NULL) are fpc_pnp_bank's.
 *  - Workspace: the pair records are two float4 each, (Qx, Qy, Qz, Tx), (Ty, Tz, row, -): the size and shape of the PnP
 *    records, so the calls use the fpc_pnp_reserve reservation for records, counts and best keys.  They allocate nothing and
 *    carve nothing; the plan hash, the packed size, the guard zones and the bank's allocations stay what they are.  A Sim(3)
 *    call overwrites the PnP pair list and the other way round; both are stream-ordered and each call packs its own list
 *    first, so neither sees the other's.
 *  - Inliers: the rule of the RETURNED model, in fp64 from the fp32 s, R, t.  With Q the query point and T the train point,
 *    Y = s R T + t and T' = R^T (Q - t) / s.  The pair is an inlier iff every coordinate of Q, T, Y and T' is finite,
 *    Yz > 0, Qz > 0, T'z > 0 and Tz > 0, and
 *        (q_fx (Yx Qz - Qx Yz))^2 + (q_fy (Yy Qz - Qy Yz))^2 < thr^2 Yz^2 Qz^2
 *        (t_fx (T'x Tz - Tx T'z))^2 + (t_fy (T'y Tz - Ty T'z))^2 < thr^2 T'z^2 Tz^2.
 *    The first asks that the transferred train point and the query's own point project within thr pixels of each other in the
 *    query camera, the second is the same test in the train camera.  No division by a depth, and in pixels: the test does not
 *    depend on either set's scale.  The principal points cancel; they stay in the struct for symmetry and are checked finite.
 *  - Sampling: mix() as above with a budget of 16 draws: r = mix(seed ^ mix((f * 4096 + t) * 16 + k)) % M; the first 3
 *    distinct indices are the sample, in that order; a hypothesis that has not found 3 within its 16 draws is degenerate.
 *  - Minimal solve, three pairs, fp64, closed form.  On each side the triad of (p0, p1, p2): d1 = p1 - p0, d2 = p2 - p0,
 *    x = d1 / |d1|, c = d1 x d2, z = c / |c|, y = z x x.  The sample is degenerate when c.c is not > 1e-12 |d1|^2 |d2|^2 on
 *    either side, or when anything is not finite.  R = [x y z]_query [x y z]_train^T (columns x, y, z).  With Qm, Tm the means
 *    of the three points, s = sqrt(sum |Q_i - Qm|^2 / sum |T_i - Tm|^2) (fix_scale: s = 1) and t = Qm - s R Tm.
 *  - Scoring: the hypothesis is rounded to fp32 as 24 values, A = s R, t, B = R^T / s and u = -R^T t / s (formed in fp64; a
 *    value that is not finite in fp32 makes the hypothesis degenerate).  Hypothesis t counts the pairs with, in fp32 (fmaf,
 *    the products added in the order x, y, z onto the translation), Y = A T + t, W = B Q + u, and both of
 *        Yz > 0, Qz > 0, (q_fx fmaf(Yx, Qz, -(Qx Yz)))^2 + (q_fy fmaf(Yy, Qz, -(Qy Yz)))^2 < (thr (Yz Qz))^2
 *        Wz > 0, Tz > 0, (t_fx fmaf(Wx, Tz, -(Tx Wz)))^2 + (t_fy fmaf(Wy, Tz, -(Ty Wz)))^2 < (thr (Wz Tz))^2
 *    where e_x^2 + e_y^2 is fmaf(e_x, e_x, e_y e_y).  Selection: the largest count; ties go to the lower t.
 *  - The best sample's model is its s, R, t rounded to fp32.  Refit, `refits` times, in fp64 (Horn's closed form): over the
 *    inliers of the current fp32 model, a first pass gives their number n and the centroids Qm, Tm; a second pass gives
 *    S = sum a b^T (9 sums), sum |a|^2 and sum |b|^2 with a = T - Tm, b = Q - Qm, accumulated in a fixed order (no
 *    floating-point atomics).  With S's entries named Sxx .. Szz (row: a's component, column: b's) the symmetric matrix
 *        N = [Sxx+Syy+Szz  Syz-Szy       Szx-Sxz       Sxy-Syx    ]
 *            [             Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz    ]
 *            [                          -Sxx+Syy-Szz   Syz+Szy    ]
 *            [                                        -Sxx-Syy+Szz]
 *    is diagonalised by the cyclic Jacobi of the fundamental section at N = 4; the eigenvector of the largest eigenvalue
 *    lambda0 (ties: the lowest index), normalised, is the unit quaternion (w, x, y, z), and
 *        R = [w^2+x^2-y^2-z^2  2(xy-wz)         2(xz+wy)        ]
 *            [2(xy+wz)         w^2-x^2+y^2-z^2  2(yz-wx)        ]
 *            [2(xz-wy)         2(yz+wx)         w^2-x^2-y^2+z^2 ],
 *    s = sqrt(sum |b|^2 / sum |a|^2) (fix_scale: 1), t = Qm - s R Tm; all rounded to fp32.  The sums are unweighted.  The
 *    refit is singular with n < 3, with sum |a|^2 or sum |b|^2 not > 0, with lambda0 - lambda1 not > 1e-12 sqrt(sum |a|^2
 *    sum |b|^2) (lambda1 the second largest: collinear inliers leave the rotation about their line free), or with a result
 *    that is not finite or an s that is not > 0 in fp32.  A singular refit keeps the model and ends the refits.
 *    A refit that returns the model it started from, value for value, also ends the refits: the same model has the same
 *    inliers and the same sums, so every further refit would return it again -- the result is that of all `refits` refits.
 *    MONOTONE GUARD: the refitted model replaces the current one only if its inlier count is not below the current model's;
 *    otherwise the current model stays and the refits end.  (A least-squares fit over inliers of noisy 3-D points can lose
 *    pairs the best sample had; the guard makes the returned count a maximum over the models visited.)
 *  - Failure: a frame with fewer than 3 pairs, with no non-degenerate sample, or with fewer than min_inliers inliers after the
 *    last refit gets s = 0, nine zeros, three zeros, ninliers = 0 and an all-zero mask.
 *  - Determinism, execution: as for the PnP calls.  The three entry points give bit-identical outputs on equal pair lists,
 *    and fpc_sim3_bank is bit-identical to fpc_sim3_frames with that slot's landmarks at the SAME frame index.  Asynchronous
 *    on the ctx stream: no host synchronisation, no device-to-host copy, no allocation; every count and slot is read on the
 *    device.  They work on a FPC_BANK_BF16 bank: they read counts and landmarks only.  fpc_detect, fpc_match_bank,
 *    fpc_pnp_bank, fpc_landmarks_bank (the frame's own landmarks), fpc_match_bank against the loop candidate, fpc_sim3_bank
 *    needs no host call in between.
 * FPC_E_INVALID (nothing is written): everything the PnP twins refuse for the arguments they share (n, stride, npairs_dev,
 * match_dev, no PnP reservation); NULL params, q_xyz_dev, s_dev, R_dev, t_dev or ninliers_dev; fpc_ransac_sim3: a NULL
 * t_xyz_dev; a focal length that is not > 0 or a non-finite intrinsic on either side; iterations outside 1 .. 4096;
 * reproj_threshold not > 0 (or not below 1e18); refits outside 0 .. 4; min_inliers < 3; fix_scale not 0 or 1;
 * fpc_sim3_frames: a NULL key_xyz_dev or nkey_dev; fpc_sim3_bank: no bank or a NULL slot_dev. */
typedef struct fpc_sim3_params {
  float q_fx, q_fy, q_cx, q_cy;   /* camera of the query side, pixels, fx, fy > 0                                         */
  float t_fx, t_fy, t_cx, t_cy;   /* camera of the train side                                                             */
  int iterations;                 /* 1 .. 4096                                                                            */
  float reproj_threshold;         /* px, > 0, below 1e18                                                                  */
  uint32_t seed;
  int refits;                     /* 0 .. 4 Horn refits on the inlier set                                                 */
  int min_inliers;                /* >= 3                                                                                 */
  int fix_scale;                  /* 0: estimate s;  1: s = 1 (rigid alignment, two sets at one scale)                    */
} fpc_sim3_params;
/* fx = fy = 500, centre (320, 240) on both sides, 1024 iterations, 3.0 px, seed 0, 4 refits, 12 inliers, fix_scale 0 */
int fpc_default_sim3_params(fpc_sim3_params* params);
int fpc_ransac_sim3(fpc_ctx* ctx, int n, const float* q_xyz_dev, const float* t_xyz_dev, const int32_t* npairs_dev, int stride,
                    const fpc_sim3_params* params, float* s_dev, float* R_dev, float* t_dev, int32_t* ninliers_dev,
                    uint8_t* inlier_dev);
int fpc_sim3_frames(fpc_ctx* ctx, int n, const float* q_xyz_dev, const uint8_t* q_valid_dev, const float* key_xyz_dev,
                    const uint8_t* key_valid_dev, const int32_t* nkey_dev, const int32_t* match_dev,
                    const fpc_sim3_params* params, float* s_dev, float* R_dev, float* t_dev, int32_t* ninliers_dev,
                    uint8_t* inlier_dev);
int fpc_sim3_bank(fpc_ctx* ctx, int n, const float* q_xyz_dev, const uint8_t* q_valid_dev, const int32_t* slot_dev,
                  const int32_t* match_dev, const fpc_sim3_params* params, float* s_dev, float* R_dev, float* t_dev,
                  int32_t* ninliers_dev, uint8_t* inlier_dev);

/* --- pose graph over the bank's slots: spread a loop's error over the key frames ---------------------------------------------
 * fpc_pnp_bank gives an odometry edge between a new key frame and the slot it was localised against, fpc_sim3_bank a loop
 * edge with the drift of the scale.  The calls below keep one Sim(3) node per bank slot and those edges on the device, spread
 * a loop's error over the nodes by Levenberg-Marquardt, and bring the bank's landmarks to one scale afterwards; nothing of it
 * needs a host round trip.  The rule is pinned by planted ring scenes and by a float64 restatement (tests/test_pose_graph.py).
 *  - Storage.  fpc_graph_reserve(ctx, nodes, edges, &bytes): 1 <= nodes <= FPC_BANK_MAX_SLOTS, 1 <= edges <=
 *    FPC_GRAPH_MAX_EDGES; the only call here that allocates or synchronises; an allocation of its own, with guard zones under
 *    FPC_PLAN_GUARD_ZONES, freed by fpc_destroy; a second reserve is FPC_E_INVALID.  It carves nothing: the plan hash, the
 *    packed size and fpc_bank_get().bytes stay what they are.  It needs no bank.  After it every node is unset and there is no
 *    edge.
 *  - Nodes.  Node i is (s_i, R_i, t_i), fp32, with X_i = s_i R_i X_w + t_i: the PnP direction with a scale.  A node is SET iff
 *    s_i > 0 (0, the cleared value, a negative or a NaN is unset: outside the problem).  fpc_graph_set_nodes writes nodes
 *    first .. first + count - 1 from device arrays s_dev float32 [count] (NULL: every s = 1), R_dev float32 [count][9]
 *    row-major, t_dev float32 [count][3], as given.  fpc_graph_clear unsets every node and empties the edges and both counters.
 *    fpc_graph_get returns device pointers into the reservation: the nodes, the edges (from, to, s, R, t, w), and count_dev
 *    int32 [2]: the edges held and the edges dropped for want of room.
 *  - Edges.  The measurement of an edge is X_to = s R X_from + t, exactly as fpc_pnp_* (s = 1) and fpc_sim3_* write it: the
 *    train slot is `from`, the slot the query frame was or will be stored in is `to`.  fpc_graph_add_edges looks at candidates
 *    f = 0 .. n - 1 (1 <= n <= FPC_GRAPH_MAX_EDGES): from_dev, to_dev int32 [n], s_dev float32 [n] or NULL (s = 1), R_dev
 *    float32 [n][9], t_dev float32 [n][3], ninliers_dev int32 [n] or NULL.  Candidate f is TAKEN iff from and to lie in
 *    [0, nodes) and differ, every value of s, R, t is finite, s > 0, R is not all zero (nine zeros are the failure output of
 *    the RANSAC calls), and ninliers_dev is NULL or ninliers[f] >= min_inliers.  Its weight w is 1 without ninliers_dev,
 *    otherwise (float)ninliers[f].  Taken candidates are appended in ascending f at count + rank (the rank is a ballot /
 *    popcount prefix: independent of the execution order); those that would land at or beyond the capacity are dropped and
 *    counted in count_dev[1].  With FPC_GRAPH_INIT_TO one lane then walks the edges THIS call appended, in ascending order:
 *    where `from` is set and `to` is not, node[to] = M o node[from] = (s s_a, R R_a, s R t_a + t), formed in fp64 and rounded
 *    to fp32 (skipped if a value is not finite in fp32 or the scale is not > 0) -- a chain of odometry edges in one batch
 *    gets its starting values without a host call.
 * The optimiser, fpc_graph_optimise(ctx, fixed_dev, params, stats_dev).  Everything is fp64 unless said otherwise; no
 * floating-point atomics; no contraction of a product and a sum.
 *  - Problem.  The ACTIVE edges are those held whose two ends are both set.  The unknowns are the set nodes with at least one
 *    active edge, except the gauge fixed_dev[0] (read on the device), which stays as it is.  A gauge outside [0, nodes) or
 *    unset makes the call FAIL: no node is written and the stats are zero.  Set nodes without an active edge, and unset
 *    nodes, never change.
 *  - Residual of edge (a, b, M = (s, R, t)) from the fp32 state: Q = R_a R_b^T, k = s_a / s_b, u = t_a - k Q t_b,
 *        E = M o S_a o S_b^-1 = (s_E, R_E, t_E) = (s k, R Q, s R u + t),
 *        e = (log R_E, t_E iu, ln s_E),  iu = 1 / trans_unit,
 *    with log R_E = (theta / |v|) v for v = vee(R_E - R_E^T) / 2 and theta = atan2(|v|, (tr R_E - 1) / 2) (v itself where
 *    |v| < 1e-12; the residual rotation is assumed away from pi).  trans_unit > 0 puts the translation in the map's units.
 *    Cost C = sum_e w_e |e|^2 (the seven squares added in order onto 0, then times w): the edges of a chunk of 64 edge
 *    indices in ascending order (an edge that is not active is a +0 term), the chunks in ascending order.
 *  - Perturbation: the PnP refit's left perturbation with a scale, S <- D(delta) S with delta = (omega, upsilon, sigma) and
 *    D = (e^sigma, E(omega), upsilon): R' = E(omega) R, t' = e^sigma E(omega) t + upsilon, s' = e^sigma s, E as in the PnP
 *    refit.
 *  - Jacobians, first order, the SO(3) log's Jacobian taken as the identity.  With d = t - t_E ([t]x - [t_E]x = [d]x):
 *        J_a = [ R          0        0    ]        J_b = [ -R_E    0            0 ]
 *              [ [d]x R iu  s R iu  -d iu ]              [  0     -s_E R_E iu   0 ]
 *              [ 0          0        1    ]              [  0      0           -1 ]
 *  - Normal equations.  Node i's gradient g_i = sum w J^T e and block H_ii = sum w J^T J run over its active edges in
 *    ascending edge index (J is J_a where i is the edge's `from`, J_b where it is its `to`).  The system is
 *    (H + lambda diag H) delta = -g with H = sum_e w [J_a J_b]^T [J_a J_b] over the unknowns (the gauge's columns left out).
 *  - Linear solve: block-Jacobi preconditioned conjugate gradients.  M_i = (H_ii + lambda diag H_ii)^-1 by Gauss-Jordan on
 *    the 7 x 14 tableau with partial pivoting (the first largest pivot, the pivot row scaled by the pivot's reciprocal); a
 *    pivot not above 1e-14 of the largest diagonal entry of the damped block, at any node, rejects the attempt.  x = 0,
 *    r = -g, z = M r, p = z, rz = rz0 = r.z; rz0 not > 0 ends the solve with x = 0.  Then at most cg_iterations times:
 *    q = A p; pq = p.q; pq not > 0 ends the solve; alpha = rz / pq; x += alpha p; r -= alpha q; z = M r; rz' = r.z;
 *    rz' <= cg_tol^2 rz0 ends the solve; p = z + (rz' / rz) p; rz = rz'.  (A p)_i is the sum over node i's active edges, in
 *    ascending edge index, of J_i^T (w (J_a p_a + J_b p_b)), plus lambda diag(H_ii) p_i.  A dot product: node i's seven products
 *    added in order onto 0, then the FIXED TREE over node indices 0 .. 1023 (a node that is no unknown is a +0 leaf): for
 *    h = 512, 256, .. 1: leaf[i] += leaf[i + h] for every i < h; the result is leaf[0].  A truncated solve is still a valid
 *    attempt: the accept rule guards the cost.
 *  - Step: S_i <- D(x_i) S_i for every unknown, rounded to fp32 (a value that is not finite in fp32 or a scale that is not > 0
 *    rejects the attempt); C' is evaluated from the rounded state.
 *  - Accept, reject, stop: the refine and window sections' rule -- accepted iff C' < C, then lambda <- max(lambda / 10, 1e-10);
 *    otherwise the state is kept and lambda <- min(10 lambda, 1e6).  The call stops after `iterations` attempts, or after an
 *    accepted step with C - C' <= 1e-6 C.
 *  - Result: the nodes in place and stats_dev float32 [4]: cost before, cost after, attempts made, attempts accepted.  A call
 *    never raises the cost; a call without an accepted attempt leaves the nodes bit for bit.
 * fpc_graph_apply_scale needs a bank with a landmark reservation and nodes == the bank's slots.  With sigma_i = s_i for a set
 * node and 1 otherwise: every held edge becomes (s sigma_a / sigma_b, R, t / sigma_b); every valid landmark row (row < the
 * slot's count, w != 0) of a set node with s_i != 1 is multiplied by 1 / s_i (the reciprocal in fp64, products rounded to fp32,
 * w kept); that node becomes (1, R_i, t_i (1 / s_i)).  Every world point R_i^T (X - t_i) / s_i of a slot is unchanged, and so
 * are the e_omega and e_sigma of every edge; t_E becomes t_E / sigma_b, so an edge's translation residual is rescaled with its
 * `to` node (zero stays zero; trans_unit is in the new units).  After it PnP against neighbouring slots returns poses at one
 * scale.  It works on both bank formats: it reads counts and reads and writes landmarks only.
 * Execution: fpc_graph_set_nodes, _clear, _add_edges, _optimise and _apply_scale are asynchronous on the ctx stream: no host
 * synchronisation, no device-to-host copy, no allocation; every count is read on the device; the optimiser is a fixed
 * sequence of launches per attempt, `iterations` times, which a device flag turns into no-ops once the call has stopped (no
 * cooperative launch, no workgroup waits on another); the conjugate-gradient solve of an attempt runs inside one workgroup,
 * a node per thread.  Repeated sequences give bit-identical results.  fpc_sim3_bank, fpc_graph_add_edges, fpc_graph_optimise,
 * fpc_graph_apply_scale needs no host call in between.
 *  - Not here: robust kernels on edges, 7 x 7 information matrices, more than FPC_BANK_MAX_SLOTS nodes, merging duplicate
 *    landmarks across slots, global bundle adjustment.
 * FPC_E_INVALID (nothing is written): every call but fpc_graph_reserve without a reservation; fpc_graph_reserve: nodes or
 * edges outside their ranges, a second reserve; fpc_graph_get: a NULL view; fpc_graph_set_nodes: a NULL R_dev or t_dev, first
 * < 0, count < 1, first + count > nodes; fpc_graph_add_edges: n outside 1 .. FPC_GRAPH_MAX_EDGES, a NULL from_dev, to_dev,
 * R_dev or t_dev, a flag other than FPC_GRAPH_INIT_TO; fpc_graph_optimise: a NULL fixed_dev, params or stats_dev, iterations
 * outside 1 .. 16, lambda0 not > 0 or not finite, cg_iterations outside 1 .. 1024, cg_tol < 0 or not finite, trans_unit not
 * > 0 or not finite; fpc_graph_apply_scale: no bank, no landmark reservation, nodes != slots. */
#define FPC_GRAPH_MAX_EDGES 16384
#define FPC_GRAPH_INIT_TO 1u
typedef struct fpc_graph_params {
  int   iterations;               /* 1 .. 16 attempts                                                                     */
  float lambda0;                  /* > 0, finite: the first damping                                                       */
  int   cg_iterations;            /* 1 .. 1024 conjugate-gradient iterations per attempt                                  */
  float cg_tol;                   /* >= 0, finite: the solve ends when r.z <= cg_tol^2 of its first value                 */
  float trans_unit;               /* > 0, finite: the length that weighs like one radian and one e-fold of scale         */
} fpc_graph_params;
typedef struct fpc_graph_view {
  int nodes, edges;               /* the capacities of the reservation                                                    */
  float* node_s;                  /* [nodes]                                                                              */
  float* node_R;                  /* [nodes][9]                                                                           */
  float* node_t;                  /* [nodes][3]                                                                           */
  int32_t* edge_from;             /* [edges]                                                                              */
  int32_t* edge_to;               /* [edges]                                                                              */
  float* edge_s;                  /* [edges]                                                                              */
  float* edge_R;                  /* [edges][9]                                                                           */
  float* edge_t;                  /* [edges][3]                                                                           */
  float* edge_w;                  /* [edges]                                                                              */
  int32_t* count;                 /* [2]: edges held, edges dropped                                                       */
  size_t bytes;                   /* allocated                                                                            */
} fpc_graph_view;
/* iterations 16, lambda0 1e-3, cg_iterations 256, cg_tol 1e-8, trans_unit 1 */
int fpc_default_graph_params(fpc_graph_params* params);
int fpc_graph_reserve(fpc_ctx* ctx, int nodes, int edges, size_t* bytes);
int fpc_graph_get(fpc_ctx* ctx, fpc_graph_view* view);
int fpc_graph_clear(fpc_ctx* ctx);
int fpc_graph_set_nodes(fpc_ctx* ctx, int first, int count, const float* s_dev, const float* R_dev, const float* t_dev);
int fpc_graph_add_edges(fpc_ctx* ctx, int n, const int32_t* from_dev, const int32_t* to_dev, const float* s_dev,
                        const float* R_dev, const float* t_dev, const int32_t* ninliers_dev, int min_inliers, unsigned flags);
int fpc_graph_optimise(fpc_ctx* ctx, const int32_t* fixed_dev, const fpc_graph_params* params, float* stats_dev);
int fpc_graph_apply_scale(fpc_ctx* ctx);

int fpc_results(fpc_ctx* ctx, fpc_device_results* out);
/* Synchronises, then copies the per-frame counts to the host.  FPC_E_NONFINITE (counts delivered all the same) when a
 * frame of the call held a NaN / Inf pixel: "Numerical contract" at the top of this header. */
int fpc_get_counts(fpc_ctx* ctx, int n, int32_t* count_host, int32_t* n_candidates_host);
/* Synchronises; per frame of the last call: the largest logit (fpc_detect and fpc_forward; logits are post-ReLU, >= 0),
 * the largest |value| of the descriptor map (fpc_forward with a desc output only, else 0; a frame's figure may include
 * its neighbour's -- it bounds the tensor), and whether the frame held a non-finite pixel (FPC_F32 only).  Host arrays of
 * n entries, any may be NULL.  What the "Numerical contract" above is checked against. */
int fpc_output_range(fpc_ctx* ctx, int n, float* max_logit_host, float* max_desc_host, int32_t* nonfinite_input_host);
/* Synchronises, then copies frame `frame`'s keypoints: xy [K][2], conf [K],
 * desc [K][128] (desc may be NULL).  Returns K, or FPC_E_CAPACITY if K > cap
 * (nothing is written then; fpc_get_counts gives the size). */
int fpc_get_keypoints(fpc_ctx* ctx, int frame, int cap, int32_t* xy, float* conf, float* desc);

/* Optional per-launch timing for the bench: with `enable`, every kernel launch of
 * fpc_detect / fpc_forward is bracketed by HIP events on the launch stream; records
 * accumulate over calls until the next fpc_set_timing.  enable = n > 1: only every n-th pass over a batch (the first one
 * included; one pass per fpc_detect / fpc_forward / fpc_detect_u8* call, 1 + num per fpc_homography_adaptation) carries
 * the events -- two event records per launch cost 0.7 % of the frame rate at 32 VGA frames per call. */
int fpc_set_timing(fpc_ctx* ctx, int enable);
/* After fpc_sync: number of launches recorded since fpc_set_timing; names[i] (layer) and
 * kernels[i] (kernel symbol, as rocprofv3 prints it) point into ctx-owned storage;
 * ms[i] is the event-to-event duration; flops[i] the ALGORITHMIC FLOPs of that launch
 * (2 x MACs of the direct convolution x its frames, 0 for non-conv kernels); mfma_flops[i]
 * the FLOPs actually issued on the matrix cores (tile / channel padding included;
 * Winograd launches issue 16/36 of their 3x3 convolution's count); bytes[i] the ALGORITHMIC HBM bytes of that launch
 * (its input tensor(s) read once + its output tensor written once, in the mode's storage type, x its frames; weights
 * -- L2-resident -- and data-dependent post-processing traffic not counted).  Any array may be NULL. */
int fpc_get_timings(fpc_ctx* ctx, int cap, const char** names, const char** kernels, float* ms,
                    double* flops, double* mfma_flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* FPC_H */
