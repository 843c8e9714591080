// mesh_simplify_kernels.h -- the quadric vertex clustering of the mesh simplification (mesh_ops.hip: dgs_simplify_accumulate,
// dgs_simplify_solve).
// include/dgs_mesh_ops.h states the arithmetic; every sum is an exact int64 addition, so the grouping below cannot change a bit.
// A row of a cluster is SUM_ROW = 16 int64 = 128 contiguous bytes: column 0 count, 1..3 position, 4..6 colour, 7..12 A (xx xy xz yy
// yz zz), 13..15 b.  The vertex kernel adds columns 0..6, the face kernel columns 7..15.
// COMBINING ON CHIP.  A naive scatter is one 8-byte atomic per lane and column, 64 lanes in up to 64 rows: the slowest shape there
// is.  Marching tetrahedra emits vertices and faces in cell order, so neighbouring items mostly share a cluster: a workgroup hands
// its 256 items to sum_combine (mesh_common.h), which sends one atomic per run of equal neighbouring keys and column.
// Items past the end and ids outside their range carry the key -1: they take part in every barrier and are skipped at the atomic,
// which is the index guard -- no address is formed from such an id.
#pragma once
#include "mesh_common.h"

namespace {

constexpr int SIMP_THREADS = 256, SIMP_ITEMS_PER_THREAD = 1, SIMP_Q = 24, SIMP_W_MAX = 16, SIMP_LAMBDA_EXP = QUADRIC_LAMBDA_EXP;
constexpr int SIMP_POS_BITS = 30, SIMP_COL_BITS = 24;
static_assert(SIMP_THREADS == SUM_THREADS, "sum_combine is built for the workgroup these kernels launch with");

__device__ __forceinline__ long long simp_fixed(float x, float scale) { return fixed_round(x * scale); }   // scale = 2^k: the product is exact

__global__ __launch_bounds__(SIMP_THREADS) void simp_vertex_kernel(long long n_vertices, const float* __restrict__ vertices,
                                                                   const float* __restrict__ colors, const int* __restrict__ cluster,
                                                                   long long n_clusters, const float* __restrict__ centres, float cell,
                                                                   long long* __restrict__ rows) {
    __shared__ SumShared<7> sh;
    const long long i = (long long)blockIdx.x * SIMP_THREADS + threadIdx.x;
    int key = -1;
    long long v[7] = {0, 0, 0, 0, 0, 0, 0};
    if (i < n_vertices) {
        const int k = cluster[i];
        if (k >= 0 && k < n_clusters) {
            key = k;
            v[0] = 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) v[1 + a] = simp_fixed((vertices[3 * i + a] - centres[3 * (long long)k + a]) / cell, (float)(1 << SIMP_POS_BITS));
            if (colors) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float c = colors[3 * i + a];
                    v[4 + a] = simp_fixed(c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f, (float)(1 << SIMP_COL_BITS));   // NaN counts as 0
                }
            }
        }
    }
    sum_combine<7, 0>(sh, key, v, n_clusters, rows);
}

__global__ __launch_bounds__(SIMP_THREADS) void simp_face_kernel(long long n_faces, const int* __restrict__ faces, long long n_vertices,
                                                                 const float* __restrict__ vertices, const int* __restrict__ cluster,
                                                                 long long n_clusters, const float* __restrict__ centres, float cell,
                                                                 long long* __restrict__ rows) {
    __shared__ SumShared<9> sh;
    const long long i = (long long)blockIdx.x * SIMP_THREADS + threadIdx.x;
    bool ok = false;
    int k[3] = {-1, -1, -1};
    float p[3][3], nh[3] = {0.0f, 0.0f, 0.0f}, w = 0.0f;
    if (i < n_faces) {
        const int f0 = faces[3 * i], f1 = faces[3 * i + 1], f2 = faces[3 * i + 2];
        if (f0 >= 0 && f0 < n_vertices && f1 >= 0 && f1 < n_vertices && f2 >= 0 && f2 < n_vertices) {   // index guard
            const int f[3] = {f0, f1, f2};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                k[c] = cluster[f[c]];
#pragma unroll
                for (int a = 0; a < 3; ++a) p[c][a] = vertices[3 * (long long)f[c] + a];
            }
            float n[3];
            const float l = face_normal(p, n);
            if (l > 0.0f && l < INFINITY) {                             // a face with area; NaN fails both
                ok = true;
                nh[0] = n[0] / l, nh[1] = n[1] / l, nh[2] = n[2] / l;
                w = fminf((0.5f * l) / (cell * cell), (float)SIMP_W_MAX);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                       // corner c speaks for its cluster if no earlier corner is in it
        const bool first = c == 0 || (k[c] != k[0] && (c == 1 || k[c] != k[1]));
        const bool mine = ok && first && k[c] >= 0 && k[c] < n_clusters;
        if (!__syncthreads_or(mine)) continue;                          // (uniform: the whole workgroup skips the slot)
        long long v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (mine) {
            const long long m = (k[0] == k[c]) + (k[1] == k[c]) + (k[2] == k[c]);
            const float* ctr = centres + 3 * (long long)k[c];
            const float qx = (p[c][0] - ctr[0]) / cell, qy = (p[c][1] - ctr[1]) / cell, qz = (p[c][2] - ctr[2]) / cell;
            const float d = -((nh[0] * qx + nh[1] * qy) + nh[2] * qz);
            quadric_fixed(w, w * d, nh, (float)(1 << SIMP_Q), v);
#pragma unroll
            for (int a = 0; a < 9; ++a) v[a] = m * v[a];
        }
        sum_combine<9, 7>(sh, mine ? k[c] : -1, v, n_clusters, rows);
    }
}

// One thread per cluster: the fp64 solve of include/dgs_mesh_ops.h, operation by operation.
__global__ __launch_bounds__(SIMP_THREADS) void simp_solve_kernel(long long n_clusters, const long long* __restrict__ rows,
                                                                  const float* __restrict__ centres, float cell, int placement,
                                                                  float* __restrict__ vertices, float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * SIMP_THREADS + threadIdx.x;
    if (i >= n_clusters) return;
    const long long* r = rows + i * SUM_ROW;
    const double count = (double)r[0];
    const double pden = count * (double)(1 << SIMP_POS_BITS), cden = count * (double)(1 << SIMP_COL_BITS);
    double xb[3], x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = (double)r[1 + a] / pden;                       // count 0 (a cluster no vertex names): NaN fails both tests -> 0
        xb[a] = q > -1.0 ? (q < 1.0 ? q : 1.0) : -1.0;
        if (!(q == q)) xb[a] = 0.0;
        x[a] = xb[a];
    }
    if (placement == 1) {
        const double A[6] = {(double)r[7], (double)r[8], (double)r[9], (double)r[10], (double)r[11], (double)r[12]};
        const double b[3] = {(double)r[13], (double)r[14], (double)r[15]};
        double t, det, y[3];
        quadric_solve(A, b, xb, t, det, y);
        if (t > 0.0 && det > 0.0 && det < (double)INFINITY && fabs(y[0]) <= 1.0 && fabs(y[1]) <= 1.0 && fabs(y[2]) <= 1.0)   // NaN fails
            x[0] = y[0], x[1] = y[1], x[2] = y[2];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vertices[3 * i + a] = centres[3 * i + a] + (float)x[a] * cell;
        if (colors) colors[3 * i + a] = count > 0.0 ? (float)((double)r[4 + a] / cden) : 0.0f;
    }
}

}  // namespace
