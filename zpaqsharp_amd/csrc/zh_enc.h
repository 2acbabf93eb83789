// zh_enc.h — structures shared by the host side of zpaqhip_compress_blocks (zh_compress.cpp) and the encoder kernels
// (zh_enc_generic.hip, zh_enc_cm.hip, zh_enc_chain.hip).
//
// A block's "coded sequence" is what Encoder.compress sees (Compressor.cs:156-222): the post-processor prefix
// (PASS: 0; PROG: 1, length lo, length hi, program) followed by the block's bytes.  The host lays the coded sequences of
// a batch out back to back in one device buffer; each block's coded output goes to its own slot.
//
// A block holds one or more segments (Compressor.startSegment .. endSegment, repeated): its coded sequence is then the
// concatenation of its segments' coded sequences, the prefix being part of the first, and ZhEncLaunch::segs says where each
// lies.  zh_enc_chain and zh_enc_generic walk that table; zh_enc_cm takes blocks of one segment only and reads in_off / n.
#pragma once
#include <stdint.h>

#include "zh_model.h"

#define ZH_ENC_CM_MAX_N (1u << 28)   // zh_enc_cm packs position << 4 | nibble into 32 bits
#define ZH_ENC_CM_KEYS 4096u         // (window bin, high nibble) keys of the second-nibble chains; bin = c_prev & wmask
#define ZH_ENC_CM_CHAINS (256u + ZH_ENC_CM_KEYS)

// zh_enc_chain's LDS: one ZhTables for the workgroup, then a region per wave: the model's ICM / ISSE pool (`units` KiB, a
// unit is ZhComp::small_unit's 256 words: ICM 1, ISSE 2), then what the kernel keeps per block at fixed sizes (its EncWaveLds).
#define ZH_ENC_CHAIN_LDS 163840u
#define ZH_ENC_CHAIN_TABLES 79872u       // sizeof(ZhTables)
#define ZH_ENC_CHAIN_WAVE_FIXED 13648u   // sizeof(EncWaveLds) (both asserted in zh_enc_chain.hip)
#define ZH_ENC_CHAIN_MAX_WAVES 4u        // one per SIMD
inline uint32_t zh_enc_chain_stride(uint32_t units) { return units * 1024u + ZH_ENC_CHAIN_WAVE_FIXED; }
// waves of one workgroup whose regions fit (0: not even one)
inline uint32_t zh_enc_chain_fit(uint32_t units) {
  const uint32_t w = (ZH_ENC_CHAIN_LDS - ZH_ENC_CHAIN_TABLES) / zh_enc_chain_stride(units);
  return w < ZH_ENC_CHAIN_MAX_WAVES ? w : ZH_ENC_CHAIN_MAX_WAVES;
}

struct ZhEncBlock {
  uint64_t in_off;         // coded sequence in ZhEncLaunch::in
  uint64_t n;              // its length
  uint64_t slot_off;       // output slot in ZhEncLaunch::slots
  uint64_t slot_cap;       // slot bytes; the coder counts past it but never writes past it
  uint64_t scr_off;        // zh_enc_cm: first element of this block in the list / P scratch (a coded-byte index)
  uint32_t seg0, n_seg;    // zh_enc_chain / zh_enc_generic: the block's segments, [seg0, seg0 + n_seg) of ZhEncLaunch::segs (n_seg >= 1)
};

struct ZhEncSeg {
  uint64_t in_off;         // the segment's coded sequence in ZhEncLaunch::in
  uint64_t n;              // its length; 0: the segment codes its end-of-segment bit only
};

struct ZhEncResult {
  uint64_t len;            // coded bytes the arithmetic coder produced (counted past the slot)
  int32_t status;          // 0 or a ZPAQL status from the HCOMP run (generic encoder)
  uint32_t overflow;       // len > slot_cap: the slot holds a prefix only
};

struct ZhEncLaunch {
  const uint8_t *in;
  const ZhEncBlock *blocks;
  ZhEncResult *res;
  const ZhEncSeg *segs;    // zh_enc_chain / zh_enc_generic: every block's segments, a block's back to back
  uint64_t *seg_end;       // per entry of segs: the coder's byte count (counted past the slot) right behind the segment's
                           // end-of-segment bit; the last segment's is ZhEncResult::len
  uint8_t *slots;
  uint32_t n_blocks;
  uint32_t waves;          // zh_enc_chain: encoder waves per workgroup (block size / 64); arena slot (blockIdx * waves + wave)
  // zh_enc_generic
  const ZhModel *model;
  const uint8_t *code;
  const ZhTables *tables;
  uint8_t *arena;
  uint64_t arena_stride;
  uint32_t *queue;
  uint64_t budget;
  // zh_enc_chain: bytes from one wave's LDS region to the next, and of the ICM / ISSE pool at its start
  uint32_t lds_stride;
  uint32_t lds_pool;
  // zh_enc_cm: the CM's limit (arg[1] * 4), which bits of the previous byte pick its 512-entry window, and scratch
  uint32_t limit;
  uint32_t wmask;
  uint32_t *list_a;        // per block: positions << 4 | high nibble, stably ordered by window bin
  uint32_t *list_b;        // per block: positions << 4 | low nibble, stably ordered by (window bin, high nibble)
  uint32_t *bases;         // per block: ZH_ENC_CM_KEYS + 1 run starts in list_b (bin b's run in list_a is [bases[16b], bases[16b+16]))
  uint16_t *P;             // per block: 8 probabilities (predict()*2+1) per coded byte, first coded bit first
};
