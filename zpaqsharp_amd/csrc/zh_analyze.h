// zh_analyze.h — shared by the host side of zpaqhip_gap_hist_blocks (zh_pre.cpp) and its kernel (zh_analyze.hip).
#pragma once
#include <stdint.h>

#define ZH_GAP_NR 4096u            // gaps below this are counted (LibZPAQ.cs:243); also the warm-up of a slice
#define ZH_GAP_SLICE 12288u        // bytes one lane counts; with the warm-up its walk stays below 2^16 positions

struct ZhGapLaunch {
  const uint8_t *in;         // the batch's plaintext; readable for 16 bytes past its end
  const uint64_t *in_off;    // n_blocks + 1 offsets; block b's bytes start at in + in_off[b] - base
  uint64_t base;
  uint32_t *hist;            // n_blocks x ZH_GAP_NR counters, zero before the launch
};
