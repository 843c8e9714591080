// train_common.h -- what every family header of the train-ops library shares (train_ops.hip): the thread-local error
// string behind dgs_train_ops_last_error with fail(), the launch check launched(), and the GlobalF pointer type.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& m) { g_err = m; return code; }

// Tail of every launcher: 0, or `code` with "<what>: <HIP's error string>" left for dgs_train_ops_last_error.
int launched(const char* what, int code = -4)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(code, std::string(what) + ": " + hipGetErrorString(e));
}

typedef const float __attribute__((address_space(1)))* GlobalF;   // global_load instead of flat_load for pointers that come out
                                                                  // of memory (the per-replay image slots)

}  // namespace
