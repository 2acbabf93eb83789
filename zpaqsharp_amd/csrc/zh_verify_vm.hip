// zh_verify_vm.hip — the verify pass's complete post-processor (zh_verify.h): zh_generic.hip itself, built a second time
// with the decoded bytes as its input.  Lane 0 runs PostProcessor.write over them: the translated program where
// zh_zpaql_pcomp.h has one, the ZPAQL VM of zh_core.h for everything else, a caller's own PCOMP included.
#define ZH_RAW_INPUT 1
#define ZH_GENERIC_KERNEL zh_verify_generic
#define ZH_GENERIC_LAUNCH zh_launch_verify_generic
#include "zh_generic.hip"
