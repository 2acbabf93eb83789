// zh_host.h — internal host-side declarations of libzpaqhip.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/zpaqhip.h"
#include "zh_dec_chain.h"
#include "zh_model.h"

// Kernel families known to the host only (the kernels never look at a family number): zh_model.h's, and
#define ZH_FAM_CHAIN_MID8 7u     // zh_nibble.hip: mid's shape with EIGHT mixer inputs (icm, five isse, match, icm; mix) — the level-4 text model
#define ZH_FAM_CHAIN_MIN1 8u     // zh_nibble.hip: ONE ICM on min's loop — level 4's model for barely compressible data
#define ZH_NFAM_HOST 9u

// Fail the entry point (one with `zpaqhip_err *err` in scope) on a HIP error, naming the call in err->msg.
#define HIPCHK(expr)                                                          \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      char m_[112];                                                           \
      snprintf(m_, sizeof m_, "HIP: %s (%s)", hipGetErrorString(e_), #expr);  \
      zh::set_err(err, ZPAQHIP_E_HIP, -1, -1, m_);                            \
      return ZPAQHIP_E_HIP;                                                   \
    }                                                                         \
  } while (0)

namespace zh {

// zh_tables.cpp — model-independent tables, generated and pinned against the
// reference's self-check constants (Predictor.cs:71-77) and the state-table CRC.
const ZhTables &host_tables();           // aborts the call chain via ok=false if pins fail
const ZhTablesX &host_tables_x();        // derived (zh_model.h); uploaded right behind ZhTables
bool host_tables_ok();

// zh_framing.cpp
struct ScanOut {
  std::vector<zpaqhip_block> blocks;
  std::vector<zpaqhip_segment> segs;
  size_t resume_off = 0;                  // see scan_stream
  bool hit_eof = false;
  bool stopped = false;                   // the scan ended on its ScanLimit, not at the end of the buffer
};
// Stop after a block once `max_blocks` are found, or `min_blocks` are found and they span `min_bytes` (batching of the
// streaming forms).  The default never stops early.
struct ScanLimit {
  size_t min_blocks = SIZE_MAX, min_bytes = 0, max_blocks = SIZE_MAX;
  size_t min_blocks_other = 0;            // != 0: the minimum for a batch that holds any block with other than one component
};
int scan_stream(const uint8_t *in, size_t n, ScanOut &out, zpaqhip_err *err, const ScanLimit &lim = ScanLimit());
// Parses a stream-form header (hsize[2] hh hm ph pm n COMP 0 HCOMP 0) into a
// ZhModel + padded code window.  Mirrors ZPAQL.read (ZPAQL.cs:112-156) and the
// limit checks of Predictor.init (Predictor.cs:94-167).
int build_model(const uint8_t *hdr, size_t len, ZhModel &m, std::vector<uint8_t> &code, zpaqhip_err *err);

// The lane-per-component kernels' family (zh_chain.hip, zh_enc_chain.hip) and a model's units of their ICM / ISSE pool in LDS
// (ZhComp::small_unit counts them the same way: ICM 1, ISSE 2, at most 64)
inline bool chain_family(uint32_t f) {
  return (f >= ZH_FAM_CHAIN && f <= ZH_FAM_CHAIN + 3) || f == ZH_FAM_CHAIN_MID8 || f == ZH_FAM_CHAIN_MIN1;
}
inline uint32_t chain_units(const ZhModel &m) {
  uint32_t u = 0;
  for (uint32_t i = 0; i < m.n; ++i) u += m.comp[i].type == ZH_ICM ? 1u : m.comp[i].type == ZH_ISSE ? 2u : 0u;
  return u;
}
// zh_chain.hip's several-waves kernel (zh_dec_chain.h): the most decoder waves of one workgroup (one per SIMD) whose regions fit
// next to the shared tables, and the LDS of such a workgroup.  Models outside the family get no wave.
struct DecChainPlan { uint32_t units = 0, waves = 0, lds_bytes = 0; };
inline DecChainPlan plan_dec_chain(const ZhModel &m) {
  DecChainPlan p;
  if (!chain_family(m.kind & 255u)) return p;
  p.units = chain_units(m);
  p.waves = zh_dec_chain_fit(p.units);
  p.lds_bytes = p.waves ? ZH_DEC_CHAIN_TABLES + p.waves * zh_dec_chain_stride(p.units) : 0;
  return p;
}

const char *status_message(int code);
void set_err(zpaqhip_err *err, int code, int block, int seg, const char *msg = nullptr);

// zh_sha1.cpp
void sha1(const uint8_t *p, size_t n, uint8_t out[20]);

}  // namespace zh
