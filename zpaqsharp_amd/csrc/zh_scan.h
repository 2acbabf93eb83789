// zh_scan.h — what the host driver of zpaqhip_scan_device (zh_api.cpp) launches in zh_scan.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "zh_scan_walk.h"

// pieces of the streaming pass over a stream of n bytes: positions 0 .. n, n included
inline uint64_t zh_scan_pieces(uint64_t n) { return n / ZH_SCAN_PIECE + 1; }

// cnt: 3 x zh_scan_pieces(n) words (tag hits, run starts, run ends per piece; after the call their exclusive scans),
// total: 3 words (the sums).  `in` is 4-byte aligned and readable up to n rounded up to a multiple of 4.
extern "C" hipError_t zh_launch_scan_count(const uint8_t *in, uint64_t n, uint64_t *cnt, uint64_t *total, hipStream_t stream);
extern "C" hipError_t zh_launch_scan_fill(const uint8_t *in, uint64_t n, uint64_t *cnt, uint64_t *tag, uint64_t *run_start,
                                          uint64_t *run_end, uint64_t n_tag, uint64_t n_run, hipStream_t stream);
extern "C" hipError_t zh_launch_scan_parse(const uint8_t *in, uint64_t n, const ZhScanLists *L, ZhScanRec *recs, hipStream_t stream);
extern "C" hipError_t zh_launch_scan_chain(const uint8_t *in, uint64_t n, const ZhScanLists *L, const ZhScanRec *recs,
                                           zpaqhip_block *blocks, uint64_t block_cap, ZhScanResult *res, hipStream_t stream);
extern "C" hipError_t zh_launch_scan_segments(const uint8_t *in, uint64_t n, const ZhScanLists *L, const zpaqhip_block *blocks,
                                              uint64_t n_blocks, zpaqhip_segment *segs, uint64_t seg_cap, hipStream_t stream);
