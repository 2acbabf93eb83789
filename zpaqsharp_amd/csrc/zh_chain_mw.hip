// zh_chain_mw.hip — zh_chain.hip's decoder with up to four waves per workgroup (zh_decode_chain_mw, zh_decode_chain_mw_pc;
// zh_dec_chain.h has the LDS layout).  The byte loop is zh_chain.hip's decode_chain_body, compiled here once more: this file
// only selects the kernels at that file's end.
#define ZH_CHAIN_MW_TU 1
#include "zh_chain.hip"
