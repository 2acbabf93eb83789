// zh_dec_chain.h — the LDS layout of zh_chain.hip's several-waves kernels (zh_decode_chain_mw, zh_decode_chain_mw_pc), shared
// by the host's plan (zh_host.h's plan_dec_chain, zh_api.cpp's launch) and the kernels.
//
// One ZhTables for the workgroup, then a region per wave: the ICM / ISSE pool (`units` KiB, a unit is ZhComp::small_unit's 256
// words: ICM 1, ISSE 2), then what a decoder wave keeps per block at fixed sizes (zh_chain.hip's ChainWaveLds).  The same
// carve-up as the lane-per-component encoder's (zh_enc.h); the fixed part is larger by the post-processor's memories.
#pragma once
#include <stdint.h>

#define ZH_DEC_CHAIN_LDS 163840u
#define ZH_DEC_CHAIN_TABLES 79872u       // sizeof(ZhTables)
#define ZH_DEC_CHAIN_WAVE_FIXED 16320u   // sizeof(ChainWaveLds) (both asserted in zh_chain.hip)
#define ZH_DEC_CHAIN_MAX_WAVES 4u        // one per SIMD
inline uint32_t zh_dec_chain_stride(uint32_t units) { return (units * 1024u + ZH_DEC_CHAIN_WAVE_FIXED + 15u) & ~15u; }
// waves of one workgroup whose regions fit (0: not even one)
inline uint32_t zh_dec_chain_fit(uint32_t units) {
  const uint32_t w = (ZH_DEC_CHAIN_LDS - ZH_DEC_CHAIN_TABLES) / zh_dec_chain_stride(units);
  return w < ZH_DEC_CHAIN_MAX_WAVES ? w : ZH_DEC_CHAIN_MAX_WAVES;
}

// second kernel argument of the several-waves kernels
struct ZhChainWaves {
  uint32_t waves;          // decoder waves per workgroup (block size / 64); wave w of workgroup b owns arena slot b * waves + w
  uint32_t lds_stride;     // bytes from one wave's LDS region to the next
  uint32_t lds_pool;       // bytes of the ICM / ISSE pool at the start of a region: the largest of the launch's models
};
