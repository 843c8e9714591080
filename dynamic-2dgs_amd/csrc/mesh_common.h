// mesh_common.h -- what more than one family header of the mesh library shares (mesh_ops.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

}  // namespace
