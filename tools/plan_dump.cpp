// Stand-alone driver of the launch planner (csrc/gst_plan.h) for tests/test_plan.py:
//   plan_dump large C mask debug eval_only rec_on DATASET...
//   plan_dump large_acc ...   the same call with the posterior sums on (plan_large's acc_on)
//       DATASET = npad,mp,nf,nec,ntm,ntm_pad,raug,ec_disjoint,gx_nt
//       prints "error: <message>", or per launch
//       "<prologue|sweep> <kernel> <kind> <gx> <gy> <block> <lds bytes> <kclass> <floor> <ev> <record>"
//   plan_dump persist ncu C tape eval_only mask waves NS MT K0
//       prints "wpb pair occ2 use_prog grid block tmfac_bytes"
//   plan_dump lds nf nec ntm mp ntm_pad raug
//       prints the layouts' totals in bytes: "tmelim btm hyper0 hyper1 hyper2"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gst_plan.h"

static const char* kNames[gst::LK_COUNT] = {
    "tb", "record", "white<64>", "white<256>", "white<1024>", "gram_ec<1>", "gram_ec<2>",
    "gram_ec<3>", "gram_ec<4>", "gram_small<1>", "gram_small<2>", "gram_small<3>",
    "gram_small<4>", "gram_small<5>", "gram_small<6>", "gram", "tmelim", "hyper_reg<8>",
    "hyper_reg<16>", "hyper<0>", "hyper<1>", "hyper<2>", "hyper_ecr<6,46>", "hyper_ecr<8,62>",
    "btm", "toa<256>", "toa<1024>", "accum"};
static const char* kKinds[GST_K_COUNT] = {"RECORD", "WHITE", "GRAM", "TMELIM", "HYPER", "BTM",
                                          "TB", "TOA", "ACCUM"};

static void dump(const char* list, const std::vector<gst::Launch>& v) {
  for (const gst::Launch& l : v)
    std::printf("%s %s %s %d %d %d %zu %d %d %d %d\n", list, kNames[l.kernel], kKinds[l.kind], l.gx,
                l.gy, l.block, l.lds, l.kclass, l.floor_pass, l.ev, l.record ? 1 : 0);
}

int main(int argc, char** argv) {
  auto num = [&](int i) { return (int)std::strtol(argv[i], nullptr, 0); };
  const bool acc_on = argc >= 2 && !std::strcmp(argv[1], "large_acc");
  if (argc >= 8 && (acc_on || !std::strcmp(argv[1], "large"))) {
    std::vector<gst::DevModel> mds;
    for (int i = 7; i < argc; ++i) {
      gst::DevModel md{};
      if (std::sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d,%d,%d", &md.npad, &md.mp, &md.nf, &md.nec,
                      &md.ntm, &md.ntm_pad, &md.raug, &md.ec_disjoint, &md.gx_nt) != 9)
        return 2;
      mds.push_back(md);
    }
    const gst::LargePlan p = gst::plan_large(mds.data(), (int)mds.size(), num(4), num(2),
                                             (unsigned)num(3), num(5) != 0, num(6) != 0, acc_on);
    if (!p.error.empty()) {
      std::printf("error: %s\n", p.error.c_str());
      return 0;
    }
    dump("prologue", p.prologue);
    dump("sweep", p.sweep);
    return 0;
  }
  if (argc == 11 && !std::strcmp(argv[1], "persist")) {
    const gst::PersistPlan p = gst::plan_persistent(num(2), num(3), num(4) != 0, num(5) != 0,
                                                    (unsigned)num(6), num(7), num(8), num(9), num(10));
    std::printf("%d %d %d %d %d %d %zu\n", p.wpb, p.pair ? 1 : 0, p.occ2 ? 1 : 0,
                p.use_prog ? 1 : 0, p.grid, p.block, p.tmfac_bytes);
    return 0;
  }
  if (argc == 8 && !std::strcmp(argv[1], "lds")) {
    const int nf = num(2), nec = num(3), ntm = num(4), mp = num(5);
    std::printf("%d %d %d %d %d\n", 8 * gst::TmelimLds(mp).total,
                8 * gst::BtmLds(num(6), num(7)).total, 8 * gst::HyperLds<0>(nf, nec, ntm, mp).total,
                8 * gst::HyperLds<1>(nf, nec, ntm, mp).total,
                8 * gst::HyperLds<2>(nf, nec, ntm, mp).total);
    return 0;
  }
  return 2;
}
