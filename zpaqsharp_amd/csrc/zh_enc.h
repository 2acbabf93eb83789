// zh_enc.h — structures shared by the host side of zpaqhip_compress_blocks (zh_compress.cpp) and the encoder kernels
// (zh_enc_generic.hip, zh_enc_cm.hip).
//
// A block's "coded sequence" is what Encoder.compress sees (Compressor.cs:156-222): the post-processor prefix
// (PASS: 0; PROG: 1, length lo, length hi, program) followed by the block's bytes.  The host lays the coded sequences of
// a batch out back to back in one device buffer; each block's coded output goes to its own slot.
#pragma once
#include <stdint.h>

#include "zh_model.h"

#define ZH_ENC_CM_MAX_N (1u << 28)   // zh_enc_cm packs position << 4 | nibble into 32 bits
#define ZH_ENC_CM_KEYS 4096u         // (window bin, high nibble) keys of the second-nibble chains; bin = c_prev & wmask
#define ZH_ENC_CM_CHAINS (256u + ZH_ENC_CM_KEYS)

struct ZhEncBlock {
  uint64_t in_off;         // coded sequence in ZhEncLaunch::in
  uint64_t n;              // its length
  uint64_t slot_off;       // output slot in ZhEncLaunch::slots
  uint64_t slot_cap;       // slot bytes; the coder counts past it but never writes past it
  uint64_t scr_off;        // zh_enc_cm: first element of this block in the list / P scratch (a coded-byte index)
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
  uint8_t *slots;
  uint32_t n_blocks;
  uint32_t pad0;
  // zh_enc_generic
  const ZhModel *model;
  const uint8_t *code;
  const ZhTables *tables;
  uint8_t *arena;
  uint64_t arena_stride;
  uint32_t *queue;
  uint64_t budget;
  // zh_enc_cm: the CM's limit (arg[1] * 4), which bits of the previous byte pick its 512-entry window, and scratch
  uint32_t limit;
  uint32_t wmask;
  uint32_t *list_a;        // per block: positions << 4 | high nibble, stably ordered by window bin
  uint32_t *list_b;        // per block: positions << 4 | low nibble, stably ordered by (window bin, high nibble)
  uint32_t *bases;         // per block: ZH_ENC_CM_KEYS + 1 run starts in list_b (bin b's run in list_a is [bases[16b], bases[16b+16]))
  uint16_t *P;             // per block: 8 probabilities (predict()*2+1) per coded byte, first coded bit first
};
