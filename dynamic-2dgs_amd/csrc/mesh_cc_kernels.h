// mesh_cc_kernels.h -- the connected components of the mesh clean-up (mesh_ops.hip: dgs_cc_labels).
// Lock-free union-find over label[] (include/dgs_mesh_ops.h states the contract).  INVARIANT: label[x] <= x at all times, and
// label[x] is a node of x's component.  init writes label[x] = x; the only write of the hook kernel is a successful
// atomicCAS(&label[hi], hi, lo) with lo < hi, which lowers the entry of a node that is a root at that instant; the compress kernel
// only replaces an entry by the node's root.  So every walk x -> label[x] -> ... strictly descends and ends after at most x steps at
// a node with label[r] == r.
// STALE READS.  The walks read with relaxed agent-scope atomic loads, which are served past the CU's L1.  Correctness does not rest
// on their freshness: whatever value a load returns was label[x] at some instant since the init launch, so it is an ancestor of x
// (or x) in x's component.  A walk over stale values therefore ends at an ancestor r of its start that looked like a root; whether
// it still is one is decided by the CAS alone, which executes at the memory side and returns the entry's true value.  If r has a
// parent by then, the CAS fails, writes nothing and returns that parent (< r), and the union goes on from there: after every failed
// CAS the larger of the two candidates is strictly smaller than before, so a thread cannot spin, however stale its loads are.
#pragma once
#include "mesh_common.h"

namespace {

constexpr int CC_THREADS = 256, CC_GROUPS_PER_THREAD = 1, CC_MAX_BLOCKS = 1 << 22;

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(const int* label, int x) {          // 0 <= x < n_nodes; every value read is in [0, x]
    for (int p = cc_load(label + x); p != x; p = cc_load(label + x)) x = p;
    return x;
}

__device__ __forceinline__ void cc_unite(int* label, int a, int b) {
    int ra = cc_find(label, a), rb = cc_find(label, b);
    while (ra != rb) {                                                      // equal: a and b have a common ancestor already
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicCAS(label + hi, hi, lo);
        if (old == hi) return;                                              // hi was a root and now hangs below lo
        ra = cc_find(label, old), rb = lo;                                  // old < hi is hi's true parent: go on from there
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(long long n_nodes, int* __restrict__ label) {
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_nodes; i += (long long)gridDim.x * CC_THREADS) label[i] = (int)i;
}

template <int K>
__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(long long n_nodes, const int* __restrict__ groups, long long n_groups, int* label) {
    for (long long g = (long long)blockIdx.x * CC_THREADS + threadIdx.x; g < n_groups; g += (long long)gridDim.x * CC_THREADS) {
        int anchor = -1;                                                    // the first id of the group that lies inside [0, n_nodes)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int v = groups[g * K + j];
            if (v < 0 || v >= n_nodes) continue;                            // index guard: no address below leaves label[0, n_nodes)
            if (anchor < 0) anchor = v;
            else if (v != anchor) cc_unite(label, anchor, v);
        }
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_compress_kernel(long long n_nodes, int* label) {
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n_nodes; i += (long long)gridDim.x * CC_THREADS) {
        const int p = cc_load(label + i);
        if (p == (int)i) continue;
        const int r = cc_find(label, p);
        if (r != p) __hip_atomic_store(label + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace
