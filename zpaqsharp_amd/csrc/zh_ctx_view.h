// zh_ctx_view.h — what the compress path (zh_compress.cpp) needs of a zpaqhip_ctx, whose definition stays in zh_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "zh_host.h"

namespace zh {

struct CtxView {
  int device;
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  const ZhTables *tables;       // device copy of the model-independent tables (ZhTablesX follows)
  zpaqhip_stats *stats;         // zpaqhip_last_stats
  uint32_t mem_share;           // contexts of this process sharing the device: divides the memory budget
};
CtxView ctx_view(zpaqhip_ctx *c);

}  // namespace zh
