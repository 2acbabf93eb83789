// A stand-alone drive of zh_dec_plan.h (route_block, group_blocks, arena_wish, plan_decode): the decode driver's launch plan
// without a GPU.  tests/test_dec_plan.py builds it with -fsanitize=address,undefined next to zh_framing.cpp (build_model),
// writes the cases to a file, runs it and compares every line with its own restatement of the rules.
//
// A case in the file (blank-separated tokens):
//   case NAME  has NIBBLE_MASK CHAIN2_MASK  models N HEX...  opts KERNEL MAX_CONCURRENT DEC_WAVES PP_ONLY PROF SERIAL CUS BUDGET
//   blocks N  MODEL WEIGHT ...
// (the masks: bit s set = the kernel file is built with specialisation s, what zh_nibble_has / zh_chain2_has answer in the library).
// Printed per case: its name, the arena wish, one line per group, the order of the sorted descriptors and the plan's own
// figures; or the error code.
#include <stdio.h>
#include <stdint.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "zh_dec_plan.h"

using namespace zh;

static unsigned g_nibble, g_chain2;
static int has_nibble(uint32_t spec) { return spec < 32 && (g_nibble >> spec & 1u); }
static int has_chain2(uint32_t spec) { return spec < 32 && (g_chain2 >> spec & 1u); }

static const char *kKernelName[] = {"generic", "store", "cm", "chain", "chain2", "nibble"};

static void expect(std::istream &in, const char *word) {
  std::string w;
  if (!(in >> w) || w != word) { fprintf(stderr, "case file: expected '%s', got '%s'\n", word, w.c_str()); exit(2); }
}

static void list(const char *what, const std::vector<uint32_t> &v) {
  printf("%s", what);
  for (size_t i = 0; i < v.size(); ++i) printf("%c%u", i ? ',' : '=', v[i]);
}

int main(int argc, char **argv) {
  std::ifstream file;
  if (argc > 1) file.open(argv[1]);
  std::istream &in = argc > 1 ? (std::istream &)file : std::cin;
  std::string word;
  while (in >> word) {
    if (word != "case") { fprintf(stderr, "case file: expected 'case', got '%s'\n", word.c_str()); return 2; }
    std::string name;
    in >> name;
    expect(in, "has");
    in >> g_nibble >> g_chain2;
    size_t n_models = 0, n_blocks = 0;
    expect(in, "models");
    in >> n_models;
    std::vector<ZhModel> models(n_models);
    std::vector<uint8_t> code;
    for (ZhModel &m : models) {
      std::string hex;
      in >> hex;
      std::vector<uint8_t> hdr(hex.size() / 2);
      for (size_t i = 0; i < hdr.size(); ++i) hdr[i] = (uint8_t)std::stoul(hex.substr(2 * i, 2), nullptr, 16);
      zpaqhip_err e{};
      const int rc = build_model(hdr.data(), hdr.size(), m, code, &e);
      if (rc) { fprintf(stderr, "%s: build_model %d\n", name.c_str(), rc); return 2; }
    }
    zpaqhip_opts opts{};
    opts.struct_size = sizeof opts;
    int pp_only = 0, prof = 0, serial = 0;
    uint32_t cus = 0;
    uint64_t budget = 0;
    expect(in, "opts");
    in >> opts.kernel >> opts.max_concurrent >> opts.dec_waves >> pp_only >> prof >> serial >> cus >> budget;
    expect(in, "blocks");
    in >> n_blocks;
    std::vector<ZhBlockDesc> bd(n_blocks);
    std::vector<uint64_t> weight(n_blocks);
    for (size_t k = 0; k < n_blocks; ++k) {
      in >> bd[k].model >> weight[k];
      if (bd[k].model >= n_models) { fprintf(stderr, "%s: model index\n", name.c_str()); return 2; }
      bd[k].first_seg = (uint32_t)k;                     // tells the descriptors apart in bd_sorted
    }
    if (!in) { fprintf(stderr, "%s: case file ends early\n", name.c_str()); return 2; }

    printf("case %s\n", name.c_str());
    const ZhKernelHas has = {has_nibble, has_chain2};
    std::vector<DecGroup> groups = group_blocks(models, bd, opts, pp_only != 0, has);
    printf("wish %llu\n", (unsigned long long)arena_wish(groups, opts));
    DecPlan plan;
    zpaqhip_err err{};
    const int rc = plan_decode(std::move(groups), models, bd, weight, opts, prof != 0, cus, budget, serial != 0, plan, &err);
    if (rc) { printf("error %d %d\n", rc, err.code); continue; }
    for (const DecGroup &g : plan.groups) {
      printf("group fam=%u kernel=%s spec=%u flags=%u x2=%d pcall=%d grid=%u slots=%u waves=%u pool=%u lds_stride=%u stride=%llu off=%llu base=%zu ",
             g.route.group, kKernelName[(int)g.route.kernel], g.route.spec, g.route.flags, (int)g.cm_x2, (int)g.pcall, g.grid(), g.slots,
             g.mw.waves, g.mw.lds_pool, g.mw.lds_stride, (unsigned long long)g.stride, (unsigned long long)g.arena_off, g.base);
      list("order", g.blocks);
      printf("\n");
    }
    std::vector<uint32_t> sorted;
    for (const ZhBlockDesc &b : plan.bd_sorted) sorted.push_back(b.first_seg);
    list("sorted", sorted);
    printf("\nplan side=%d arena=%llu launches=%u concurrent=%u kind=%u\n", (int)plan.side_by_side, (unsigned long long)plan.arena_bytes,
           plan.launches, plan.concurrent, plan.kernel_kind);
  }
  return 0;
}
