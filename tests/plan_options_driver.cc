// Stand-alone driver of csrc/plan_options.h for tests/test_plan_options.py: host code only, no HIP.
//
//   plan_options_driver DTYPE ARCH NUM_STREAMS PLAN_FLAGS NMS_ROUND_LAUNCHES MIN_SUB_BATCH
//
// resolves the options of that config in this process's environment and prints every field as `name=value`;
//
//   plan_options_driver grid TILES RESIDENT PARTS CAP
//
// prints bf16_persistent_grid(TILES, RESIDENT, PARTS, CAP).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "plan_options.h"

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "grid")) {
    printf("%d\n", fpc::bf16_persistent_grid(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
    return 0;
  }
  if (argc != 7) {
    fprintf(stderr, "usage: %s dtype arch num_streams plan_flags nms_round_launches min_sub_batch\n", argv[0]);
    return 2;
  }
  fpc_config cfg{};
  cfg.dtype = atoi(argv[1]);
  cfg.arch = atoi(argv[2]);
  cfg.num_streams = atoi(argv[3]);
  cfg.plan_flags = (unsigned)strtoul(argv[4], nullptr, 0);
  cfg.nms_round_launches = atoi(argv[5]);
  cfg.min_sub_batch = atoi(argv[6]);
  const fpc::PlanOptions o = fpc::resolve_plan_options(cfg, [](const char* name) -> const char* { return getenv(name); });
#define P(field) printf(#field "=%d\n", (int)o.field)
  P(fuse_blocks); P(winograd); P(winograd_gen); P(winograd_in1); P(winograd_det); P(winograd_det_gen3); P(w36_paired);
  P(latency_tiles); P(tiles_round6); P(layer1_t816); P(conv_lean); P(fuse_stem_pool); P(stem_lean); P(stem2);
  P(fuse_softmax); P(convt_fused); P(persist_min_tiles); P(xcd_order); P(w36_cus); P(bf16_grid); P(nms_one_workgroup); P(nms_passes);
  P(nms_g); P(nsub); P(nside); P(min_sub); P(split_heads); P(nms_aside); P(guard_zones);
#undef P
  return 0;
}
