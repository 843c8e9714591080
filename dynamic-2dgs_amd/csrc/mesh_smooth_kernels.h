// mesh_smooth_kernels.h -- the Jacobi step of the Laplacian / Taubin mesh smoothing (mesh_ops.hip: dgs_smooth_steps).
// include/dgs_mesh_ops.h states the step.  One launch is one Jacobi step: it reads `in` and writes `out`, two different buffers, so
// no launch reads what it writes and no workgroup waits for another.
// SHAPE.  A thread per vertex.  The sum of a row is sequential by contract (its order is its bits), so the lanes of a wave cannot
// share a row's additions; what a few lanes per vertex could share are the C channels, and at C = 3 that leaves a quarter of every
// wave idle while each lane still walks the whole row.  A thread per vertex keeps all C accumulators in registers, reads offsets,
// pinned and its own value coalesced, and reads neighbouring rows of `neighbours` from neighbouring lanes (rows are 4..10 entries, so
// a wave's rows are one contiguous piece of about 1.5 KiB).  The gather itself is 4 C bytes per neighbour at an address the mesh
// decides: marching tetrahedra numbers vertices by grid key, so a row's neighbours lie in a few nearby lines and the L2 serves most
// of them; a mesh with shuffled ids pays a line per neighbour (tools/mesh_smooth_timing.py measures both).
// The row is walked in batches of SMOOTH_BATCH: the ids of a batch are loaded, then its values, then the additions run in row
// order -- independent loads in flight, the same sequence of additions.  A row of thousands of entries (the hub of a fan) is one
// thread's loop: accepted, the meshes of this project have none.
// GUARDS.  The row range is clamped to [0, n_entries]; an id outside [0, n_vertices) adds nothing and no address is formed from it.
#pragma once
#include "mesh_common.h"

namespace {

constexpr int SMOOTH_THREADS = 256, SMOOTH_VERTS_PER_BLOCK = 256, SMOOTH_MAX_C = 8, SMOOTH_MAX_STEPS = 1024, SMOOTH_BATCH = 4;

template <int C>
__global__ __launch_bounds__(SMOOTH_THREADS) void smooth_step_kernel(long long n_vertices, const long long* __restrict__ offsets,
                                                                     const int* __restrict__ neighbours, long long n_entries, int mode, float s,
                                                                     const unsigned char* __restrict__ pinned, const float* __restrict__ in,
                                                                     float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * SMOOTH_VERTS_PER_BLOCK + threadIdx.x;
    if (i >= n_vertices) return;
    float x[C], acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = in[i * C + c], acc[c] = 0.0f;
    long long b, e;
    csr_row(offsets, i, n_entries, b, e);
    const long long d = e - b;
    if (d == 0 || (pinned && pinned[i])) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = x[c];
        return;
    }
    long long k = b;
    for (; k + SMOOTH_BATCH <= e; k += SMOOTH_BATCH) {
        int id[SMOOTH_BATCH];
        float v[SMOOTH_BATCH][C];
#pragma unroll
        for (int t = 0; t < SMOOTH_BATCH; ++t) id[t] = neighbours[k + t];
#pragma unroll
        for (int t = 0; t < SMOOTH_BATCH; ++t) {
            const bool ok = id[t] >= 0 && (long long)id[t] < n_vertices;
#pragma unroll
            for (int c = 0; c < C; ++c) v[t][c] = ok ? in[(long long)id[t] * C + c] : 0.0f;   // acc is never -0 (it starts at +0): + 0 adds nothing
        }
#pragma unroll
        for (int t = 0; t < SMOOTH_BATCH; ++t) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + v[t][c];
        }
    }
    for (; k < e; ++k) {
        const int id = neighbours[k];
        if (id >= 0 && (long long)id < n_vertices) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = acc[c] + in[(long long)id * C + c];
        }
    }
    if (mode == 0) {
        const float fd = (float)d;
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = x[c] + s * (acc[c] / fd - x[c]);
    } else {
        const float fd = (float)(d + 1);
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = (x[c] + acc[c]) / fd;
    }
}

}  // namespace
