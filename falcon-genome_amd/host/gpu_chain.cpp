#include "gpu_chain.h"

#include <dlfcn.h>

#include <string>

#include "common.h"

namespace fcsg {

namespace {

struct ChainApi {
  decltype(&fcsmm_chain) chain = nullptr;
  const char* (*last_error)() = nullptr;
  bool ok() const { return chain && last_error; }
};

const ChainApi& chain_api() {
  static const ChainApi A = [] {
    ChainApi a;
    a.chain = reinterpret_cast<decltype(a.chain)>(dlsym(RTLD_DEFAULT, "fcsmm_chain"));
    a.last_error = reinterpret_cast<decltype(a.last_error)>(dlsym(RTLD_DEFAULT, "fcs_last_error"));
    return a;
  }();
  return A;
}

}  // namespace

bool gpu_chain_available() { return chain_api().ok(); }

void gpu_chain_batch(int device, const fcsmm_batch& b, int32_t* f, int32_t* p) {
  const ChainApi& A = chain_api();
  if (!A.ok()) throw internalError("[E::fcsg] GPU chaining without its entry point");
  if (A.chain(device, &b, f, p) != 0)
    throw failedCommand(std::string("[E::fcs-genome align] chaining on GPU ") + std::to_string(device) + ": " + A.last_error());
}

}  // namespace fcsg
