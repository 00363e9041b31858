// The chaining recurrence of a chunk on the GPU (include/fcsmm.h; minimap.gpu_chain).
// The entry point is looked up in the loaded libfcship at run time, as
// gpu_seed.cpp does: a library without it, the tests' CPU mock for one, leaves
// chaining on the host (mm_chain_host).
#pragma once

#include "fcsmm.h"

namespace fcsg {

bool gpu_chain_available();
// fcsmm_chain on `device` over a batch in host memory; throws failedCommand with the library's message.
void gpu_chain_batch(int device, const fcsmm_batch& b, int32_t* f, int32_t* p);

}  // namespace fcsg
