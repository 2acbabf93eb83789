// zh_verify_lz.hip — the verify pass's wave-wide post-processors (zh_verify.h): zh_store.hip itself, built a second time
// with the decoded bytes as its input.  PASS, lazy2 and lzpre with and without E8E9, and bwtrle run here exactly as the
// decoder runs them (parser wave, flusher wave, ring, e8_pass, ibwt_block); every other program comes back as ZH_E_RETRY
// and goes to zh_verify_vm.hip.
#define ZH_RAW_INPUT 1
#define ZH_STORE_KERNEL zh_verify_store
#define ZH_STORE_LAUNCH zh_launch_verify_store
#include "zh_store.hip"
