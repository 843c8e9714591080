// mesh_cc_kernels.h -- the connected components of the mesh clean-up (mesh_ops.hip: dgs_cc_labels) and, after them, the quadric
// vertex clustering of the mesh simplification (dgs_simplify_accumulate, dgs_simplify_solve), the Jacobi step of the mesh
// smoothing (dgs_smooth_steps), the quadric edge collapse of the mesh decimation (dgs_decimate_*) and the list ranking, loop sums
// and ring emission of the hole filling (dgs_fill_*).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ---- connected components -------------------------------------------------------------------------------------------------------
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

// ---- quadric vertex clustering (mesh_ops.hip: dgs_simplify_accumulate, dgs_simplify_solve) ---------------------------------------
// include/dgs_mesh_ops.h states the arithmetic; every sum is an exact int64 addition, so the grouping below cannot change a bit.
// A row of a cluster is 16 int64 = 128 contiguous bytes: column 0 count, 1..3 position, 4..6 colour, 7..12 A (xx xy xz yy yz zz),
// 13..15 b.  The vertex kernel adds columns 0..6, the face kernel columns 7..15.
// COMBINING ON CHIP.  A naive scatter is one 8-byte atomic per lane and column, 64 lanes in up to 64 rows: the slowest shape there
// is.  Marching tetrahedra emits vertices and faces in cell order, so neighbouring items mostly share a cluster.  A workgroup
// therefore (1) stores key and values of its 256 items in LDS, (2) finds the runs of equal neighbouring keys (a head is an item whose
// left neighbour has another key; ballot + popcount number the heads, a 4-entry table joins the waves), (3) gives every run to 16
// lanes, one per column, each of which sums its column over the run out of LDS and issues ONE atomic: a wave instruction covers
// four runs, each lane group a contiguous piece (56 / 72 bytes) of one row.  Zero sums (a mesh without colours) are not sent.
// Items past the end and ids outside their range carry the key -1: they take part in every barrier and are skipped at the atomic,
// which is the index guard -- no address is formed from such an id.
constexpr int SIMP_THREADS = 256, SIMP_ITEMS_PER_THREAD = 1, SIMP_ROW = 16, SIMP_Q = 24, SIMP_W_MAX = 16, SIMP_LAMBDA_EXP = -10;
constexpr int SIMP_POS_BITS = 30, SIMP_COL_BITS = 24, SIMP_WAVES = SIMP_THREADS / 64;

template <int NCOL>
struct SimpShared {
    long long val[SIMP_THREADS][NCOL];
    int key[SIMP_THREADS];
    int start[SIMP_THREADS + 1];       // first item of every run, then SIMP_THREADS
    int wave_runs[SIMP_WAVES];
};

// Every thread of the workgroup calls this (no early exit before it).  COL0: the first of the NCOL columns these values go to.
template <int NCOL, int COL0>
__device__ __forceinline__ void simp_combine(SimpShared<NCOL>& sh, int key, const long long (&v)[NCOL], long long n_clusters,
                                             long long* __restrict__ rows) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    sh.key[t] = key;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) sh.val[t][c] = v[c];
    __syncthreads();
    const bool head = t == 0 || sh.key[t - 1] != key;
    const unsigned long long heads = __ballot(head);
    if (lane == 0) sh.wave_runs[wave] = __popcll(heads);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SIMP_WAVES; ++w) {
        const int n = sh.wave_runs[w];
        base += w < wave ? n : 0;
        total += n;
    }
    if (head) sh.start[base + __popcll(heads & ((1ull << lane) - 1ull))] = t;
    if (t == 0) sh.start[total] = SIMP_THREADS;
    __syncthreads();
    const int col = t & (SIMP_ROW - 1);
    for (int r = t / SIMP_ROW; r < total; r += SIMP_THREADS / SIMP_ROW) {
        const int s = sh.start[r], e = sh.start[r + 1], k = sh.key[s];
        if (col >= NCOL || k < 0 || k >= n_clusters) continue;          // index guard: rows[k] exists
        long long sum = 0;
        for (int i = s; i < e; ++i) sum += sh.val[i][col];
        if (sum != 0) atomicAdd((unsigned long long*)(rows + (long long)k * SIMP_ROW + COL0 + col), (unsigned long long)sum);
    }
    __syncthreads();                                                    // the buffers are free for the next call
}

__device__ __forceinline__ long long simp_fixed(float x, float scale) { return (long long)rintf(x * scale); }   // scale = 2^k: the product is exact

__global__ __launch_bounds__(SIMP_THREADS) void simp_vertex_kernel(long long n_vertices, const float* __restrict__ vertices,
                                                                   const float* __restrict__ colors, const int* __restrict__ cluster,
                                                                   long long n_clusters, const float* __restrict__ centres, float cell,
                                                                   long long* __restrict__ rows) {
    __shared__ SimpShared<7> sh;
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
    simp_combine<7, 0>(sh, key, v, n_clusters, rows);
}

__global__ __launch_bounds__(SIMP_THREADS) void simp_face_kernel(long long n_faces, const int* __restrict__ faces, long long n_vertices,
                                                                 const float* __restrict__ vertices, const int* __restrict__ cluster,
                                                                 long long n_clusters, const float* __restrict__ centres, float cell,
                                                                 long long* __restrict__ rows) {
    __shared__ SimpShared<9> sh;
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
            const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
            const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
            const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            // the length through the fp64 square root, which is correctly rounded on both sides (sqrtf is not on the device)
            const float l = (float)sqrt((double)((nx * nx + ny * ny) + nz * nz));
            if (l > 0.0f && l < INFINITY) {                             // a face with area; NaN fails both
                ok = true;
                nh[0] = nx / l, nh[1] = ny / l, nh[2] = nz / l;
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
            const float scale = (float)(1 << SIMP_Q), wd = w * d;
            int o = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = a; b < 3; ++b) v[o++] = m * simp_fixed((w * nh[a]) * nh[b], scale);
#pragma unroll
            for (int a = 0; a < 3; ++a) v[6 + a] = m * simp_fixed(wd * nh[a], scale);
        }
        simp_combine<9, 7>(sh, mine ? k[c] : -1, v, n_clusters, rows);
    }
}

// One thread per cluster: the fp64 solve of include/dgs_mesh_ops.h, operation by operation.
__global__ __launch_bounds__(SIMP_THREADS) void simp_solve_kernel(long long n_clusters, const long long* __restrict__ rows,
                                                                  const float* __restrict__ centres, float cell, int placement,
                                                                  float* __restrict__ vertices, float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * SIMP_THREADS + threadIdx.x;
    if (i >= n_clusters) return;
    const long long* r = rows + i * SIMP_ROW;
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
        const double a00 = (double)r[7], a01 = (double)r[8], a02 = (double)r[9], a11 = (double)r[10], a12 = (double)r[11], a22 = (double)r[12];
        const double t = (a00 + a11) + a22, reg = t * 0x1p-10;
        static_assert(SIMP_LAMBDA_EXP == -10, "reg above is t * 2^SIMP_LAMBDA_EXP");
        const double m00 = a00 + reg, m11 = a11 + reg, m22 = a22 + reg;
        const double r0 = reg * xb[0] - (double)r[13], r1 = reg * xb[1] - (double)r[14], r2 = reg * xb[2] - (double)r[15];
        const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
        const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
        const double det = (m00 * c00 + a01 * c01) + a02 * c02;
        if (t > 0.0 && det > 0.0 && det < (double)INFINITY) {
            const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
            const double y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
            const double y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
            if (fabs(y0) <= 1.0 && fabs(y1) <= 1.0 && fabs(y2) <= 1.0) x[0] = y0, x[1] = y1, x[2] = y2;   // NaN fails
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vertices[3 * i + a] = centres[3 * i + a] + (float)x[a] * cell;
        if (colors) colors[3 * i + a] = count > 0.0 ? (float)((double)r[4 + a] / cden) : 0.0f;
    }
}

// ---- Laplacian / Taubin smoothing (mesh_ops.hip: dgs_smooth_steps) ------------------------------------------------------------------
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
    long long b = offsets[i], e = offsets[i + 1];
    b = b < 0 ? 0 : (b > n_entries ? n_entries : b);
    e = e < b ? b : (e > n_entries ? n_entries : e);
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

// ---- quadric edge collapse in rounds (mesh_ops.hip: dgs_decimate_quadrics, _edges, _select, _apply) -----------------------------------
// include/dgs_mesh_ops.h states every step; dgs_amd/mesh_decimate.py states the same arithmetic in PyTorch.  The quadric rows are
// int64 sums (exact in any order), everything fp64 below is written operation by operation (-ffp-contract=off), and the selection
// is decided by 64-bit atomic minima of distinct keys, whose result does not depend on the order in which they land.
// SHAPE.  A thread per face (quadrics, re-indexing), per edge (cost / placement / validity, the selection passes) or per selected
// edge (apply).  The edge kernel is the heavy one: two 10-column int64 rows, an fp64 3x3 solve, a merge of two adjacency rows and a
// walk over the faces of both endpoints (about 12 faces, 9 floats each).  All of its reads are gathers at addresses the mesh
// decides; marching tetrahedra numbers vertices by grid key, so the rows of an edge's endpoints and of their faces lie in nearby
// lines and the L2 serves most of them.  A hub of thousands of faces is one thread's loop: correct, and as slow as that sounds.
// GUARDS.  Every id read from a buffer is range-checked before an address is formed from it, and every row range is clamped to its
// array: an edge, a face or a selected entry with an id outside its range computes nothing and writes its neutral output.
constexpr int DEC_THREADS = 256, DEC_ITEMS_PER_THREAD = 1, DEC_ROW = 10, DEC_Q_MAX = 40, DEC_Q_BUDGET = 59, DEC_W_MAX = 16, DEC_LAMBDA_EXP = -10;
constexpr int DEC_MIN_VALENCE = 5, DEC_LEN_BITS = 28, DEC_FLAG_LOCKED = 1, DEC_FLAG_BOUNDARY = 2;
constexpr unsigned long long DEC_NO_KEY = 0x7FFFFFFFFFFFFFFFull;

__device__ __forceinline__ bool dec_in(int id, long long n) { return id >= 0 && (long long)id < n; }

// the row [b, e) of a CSR table, clamped to [0, n_entries]
__device__ __forceinline__ void dec_row(const long long* __restrict__ offsets, int i, long long n_entries, long long& b, long long& e) {
    b = offsets[i], e = offsets[i + 1];
    b = b < 0 ? 0 : (b > n_entries ? n_entries : b);
    e = e < b ? b : (e > n_entries ? n_entries : e);
}

__device__ __forceinline__ unsigned long long dec_key(float cost, long long edge) {
    unsigned h = (unsigned)edge * 0x9E3779B1u;              // a bijection of the 32-bit integers: equal costs are ordered pseudo-randomly
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    return ((unsigned long long)__float_as_uint(cost) << 32) | h;
}

__device__ __forceinline__ void dec_cross(const double (&a)[3], const double (&b)[3], double (&n)[3]) {
    n[0] = a[1] * b[2] - a[2] * b[1], n[1] = a[2] * b[0] - a[0] * b[2], n[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(DEC_THREADS) void dec_quadric_kernel(long long n_faces, const int* __restrict__ faces, long long n_vertices,
                                                                  const float* __restrict__ pos, float mean_len, double scale,
                                                                  long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_faces) return;
    const int f[3] = {faces[3 * i], faces[3 * i + 1], faces[3 * i + 2]};
    if (!dec_in(f[0], n_vertices) || !dec_in(f[1], n_vertices) || !dec_in(f[2], n_vertices)) return;       // index guard
    float p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[c][a] = pos[3 * (long long)f[c] + a];
    const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float l = (float)sqrt((double)((nx * nx + ny * ny) + nz * nz));      // the fp64 square root: correctly rounded on both sides
    if (!(l > 0.0f && l < INFINITY)) return;                                   // a face without area counts for nothing
    const double n[3] = {(double)(nx / l), (double)(ny / l), (double)(nz / l)};
    const double w = (double)fminf(l / mean_len, (float)DEC_W_MAX);
    const double d = -((n[0] * (double)p[0][0] + n[1] * (double)p[0][1]) + n[2] * (double)p[0][2]), wd = w * d;
    long long v[DEC_ROW];
    int o = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) v[o++] = (long long)rint(((w * n[a]) * n[b]) * scale);
#pragma unroll
    for (int a = 0; a < 3; ++a) v[6 + a] = (long long)rint((wd * n[a]) * scale);
    v[9] = (long long)rint((wd * d) * scale);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < DEC_ROW; ++k)
            if (v[k] != 0) atomicAdd((unsigned long long*)(rows + (long long)f[c] * DEC_ROW + k), (unsigned long long)v[k]);
}

__global__ __launch_bounds__(DEC_THREADS) void dec_edge_kernel(long long n_vertices, const float* __restrict__ pos, const long long* __restrict__ rows,
                                                               const unsigned char* __restrict__ flags, long long n_faces,
                                                               const int* __restrict__ faces, long long n_edges, const int* __restrict__ edges,
                                                               const long long* __restrict__ adj_offsets, const int* __restrict__ adj, long long n_adj,
                                                               const long long* __restrict__ vf_offsets, const int* __restrict__ vf, long long n_vf,
                                                               double inv_scale, float max_cost, float* __restrict__ cost,
                                                               float* __restrict__ place, unsigned char* __restrict__ valid) {
    const long long e = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[e], v = edges[n_edges + e], cnt = edges[2 * n_edges + e], o0 = edges[3 * n_edges + e], o1 = edges[4 * n_edges + e];
    float c_out = 0.0f, x_out[3] = {0.0f, 0.0f, 0.0f};
    bool ok = false;
    const bool ids = dec_in(u, n_vertices) && dec_in(v, n_vertices) && u != v;                             // index guard
    const bool lu = ids && (flags[u] & DEC_FLAG_LOCKED), lv = ids && (flags[v] & DEC_FLAG_LOCKED);
    if (ids && !(lu && lv)) {
        // (b) cost and placement
        double pu[3], pv[3], mid[3], r[DEC_ROW], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pu[a] = (double)pos[3 * (long long)u + a], pv[a] = (double)pos[3 * (long long)v + a], mid[a] = (pu[a] + pv[a]) * 0.5;
#pragma unroll
        for (int k = 0; k < DEC_ROW; ++k) r[k] = (double)(rows[(long long)u * DEC_ROW + k] + rows[(long long)v * DEC_ROW + k]);
        const double a00 = r[0], a01 = r[1], a02 = r[2], a11 = r[3], a12 = r[4], a22 = r[5];
        const double t = (a00 + a11) + a22, reg = t * 0x1p-10;
        static_assert(DEC_LAMBDA_EXP == -10, "reg above is t * 2^DEC_LAMBDA_EXP");
        const double m00 = a00 + reg, m11 = a11 + reg, m22 = a22 + reg;
        const double r0 = reg * mid[0] - r[6], r1 = reg * mid[1] - r[7], r2 = reg * mid[2] - r[8];
        const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
        const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
        const double det = (m00 * c00 + a01 * c01) + a02 * c02;
        const double y[3] = {((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det};
        const double rad = (fabs(pv[0] - pu[0]) + fabs(pv[1] - pu[1])) + fabs(pv[2] - pu[2]);
        const bool good = t > 0.0 && det > 0.0 && det < (double)INFINITY && fabs(y[0] - mid[0]) <= rad && fabs(y[1] - mid[1]) <= rad &&
                          fabs(y[2] - mid[2]) <= rad;                                                       // a NaN fails
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x_out[a] = (float)(lu ? pu[a] : (lv ? pv[a] : (good ? y[a] : mid[a])));
            x[a] = (double)x_out[a];                                                                        // the cost of where the vertex will really be
        }
        const double q0 = (a00 * x[0] + a01 * x[1]) + a02 * x[2], q1 = (a01 * x[0] + a11 * x[1]) + a12 * x[2], q2 = (a02 * x[0] + a12 * x[1]) + a22 * x[2];
        const double raw = (((x[0] * q0 + x[1] * q1) + x[2] * q2) + 2.0 * ((r[6] * x[0] + r[7] * x[1]) + r[8] * x[2])) + r[9];
        c_out = (float)((raw > 0.0 ? raw : 0.0) * inv_scale);
        ok = raw == raw && c_out <= max_cost;
        // (c) validity
        if (ok) {
            const bool rim_u = flags[u] & DEC_FLAG_BOUNDARY, rim_v = flags[v] & DEC_FLAG_BOUNDARY;
            ok = cnt <= 2 && o0 != o1 && !(cnt == 2 && rim_u && rim_v);
            const int opp[2] = {o0, o1};
#pragma unroll
            for (int k = 0; k < 2; ++k) {                                                                   // valence
                if (opp[k] < 0) continue;
                if (!dec_in(opp[k], n_vertices)) { ok = false; continue; }
                long long b, en;
                dec_row(adj_offsets, opp[k], n_adj, b, en);
                ok = ok && en - b >= ((flags[opp[k]] & DEC_FLAG_BOUNDARY) ? 3 : DEC_MIN_VALENCE);
            }
        }
        if (ok) {                                                                                           // link: a merge of two ascending rows
            long long a, ae, b, be;
            dec_row(adj_offsets, u, n_adj, a, ae);
            dec_row(adj_offsets, v, n_adj, b, be);
            int n_common = 0, n_bad = 0;
            while (a < ae && b < be) {                                                                      // at most (ae - a) + (be - b) <= 2 n_adj steps
                const int s = adj[a], w = adj[b];
                if (s == w) {
                    ++n_common;
                    n_bad += s != o0 && s != o1;
                    ++a, ++b;
                } else if (s < w) ++a;
                else ++b;
            }
            ok = n_common == cnt && n_bad == 0;
        }
        for (int side = 0; side < 2 && ok; ++side) {                                                        // flip: the faces at u, then at v
            long long b, en;
            dec_row(vf_offsets, side ? v : u, n_vf, b, en);
            for (long long k = b; k < en && ok; ++k) {
                const int g = vf[k];
                if (!dec_in(g, n_faces)) { ok = false; break; }
                const int f[3] = {faces[3 * (long long)g], faces[3 * (long long)g + 1], faces[3 * (long long)g + 2]};
                if (!dec_in(f[0], n_vertices) || !dec_in(f[1], n_vertices) || !dec_in(f[2], n_vertices)) { ok = false; break; }
                const bool has_u = f[0] == u || f[1] == u || f[2] == u, has_v = f[0] == v || f[1] == v || f[2] == v;
                if (has_u && has_v) continue;                                                               // the face goes with the edge
                double p[3][3], q[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool moves = f[c] == u || f[c] == v;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        p[c][a] = (double)pos[3 * (long long)f[c] + a];
                        q[c][a] = moves ? x[a] : p[c][a];
                    }
                }
                const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const double g1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]}, g2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
                double n0[3], n1[3];
                dec_cross(e1, e2, n0);
                dec_cross(g1, g2, n1);
                ok = (n0[0] * n1[0] + n0[1] * n1[1]) + n0[2] * n1[2] > 0.0;                                 // zero area afterwards, or a NaN, fails
            }
        }
    }
    cost[e] = c_out;
#pragma unroll
    for (int a = 0; a < 3; ++a) place[3 * e + a] = x_out[a];
    valid[e] = ok ? 1 : 0;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_fill_kernel(long long n, unsigned long long* __restrict__ m, unsigned long long value) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i < n) m[i] = value;
}

// The 64-bit atomic minimum behind a plain load: entries only fall during a launch, so a stale read is too large and costs an atomic
// that changes nothing -- never a missed one.
__device__ __forceinline__ void dec_min(unsigned long long* p, unsigned long long key) {
    if (key < *p) atomicMin(p, key);
}

// pass 1 (PASS == 1): m1[x] = min of the keys of the competing edges at x.  pass 2 (PASS == 2), over ALL edges, m2 a copy of m1:
// m2[x] = min(m1[x], m1[y] for y adjacent to x).  pass 3: selected iff competing and m2[u] == m2[v] == key.
template <int PASS>
__global__ __launch_bounds__(DEC_THREADS) void dec_select_kernel(long long n_vertices, long long n_edges, const int* __restrict__ edges,
                                                                 const float* __restrict__ cost, const unsigned char* __restrict__ compete,
                                                                 unsigned long long* m1, unsigned long long* m2, unsigned char* __restrict__ selected) {
    const long long e = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (e >= n_edges) return;
    const int u = edges[e], v = edges[n_edges + e];
    const bool ids = dec_in(u, n_vertices) && dec_in(v, n_vertices);                                        // index guard
    if (PASS == 1) {
        if (!ids || !compete[e]) return;
        const unsigned long long key = dec_key(cost[e], e);
        dec_min(m1 + u, key);
        dec_min(m1 + v, key);
    } else if (PASS == 2) {
        if (!ids) return;
        dec_min(m2 + u, m1[v]);
        dec_min(m2 + v, m1[u]);
    } else {
        bool s = false;
        if (ids && compete[e]) {
            const unsigned long long key = dec_key(cost[e], e);
            s = m2[u] == key && m2[v] == key;
        }
        selected[e] = s ? 1 : 0;
    }
}

__global__ __launch_bounds__(DEC_THREADS) void dec_iota_kernel(long long n, int* __restrict__ vmap) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i < n) vmap[i] = (int)i;
}

// A thread per selected edge.  The selected edges share no endpoint, so no two threads touch one vertex; a thread reads everything
// it needs of both endpoints before it writes.  (A list that names an edge twice would write the same values twice.)
__global__ __launch_bounds__(DEC_THREADS) void dec_collapse_kernel(long long n_vertices, float* pos, long long* rows, float* colors,
                                                                   const unsigned char* __restrict__ flags, unsigned char* moved, int* vmap,
                                                                   long long n_edges, const int* __restrict__ edges, const float* __restrict__ place,
                                                                   long long n_sel, const int* __restrict__ sel) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_sel) return;
    const int e = sel[i];
    if (!dec_in(e, n_edges)) return;                                                                        // index guard
    const int u = edges[e], v = edges[n_edges + e];
    if (!dec_in(u, n_vertices) || !dec_in(v, n_vertices) || u == v) return;
    const bool lu = flags[u] & DEC_FLAG_LOCKED, lv = flags[v] & DEC_FLAG_LOCKED;
    const int s = lv && !lu ? v : u, d = lv && !lu ? u : v;             // the survivor: the smaller id, unless only the larger one is locked
    float x[3], pu[3], pv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = place[3 * (long long)e + a], pu[a] = pos[3 * (long long)u + a], pv[a] = pos[3 * (long long)v + a];
    long long sum[DEC_ROW];
#pragma unroll
    for (int k = 0; k < DEC_ROW; ++k) sum[k] = rows[(long long)u * DEC_ROW + k] + rows[(long long)v * DEC_ROW + k];
    if (colors) {
        const double dl[3] = {(double)pv[0] - (double)pu[0], (double)pv[1] - (double)pu[1], (double)pv[2] - (double)pu[2]};
        const double xr[3] = {(double)x[0] - (double)pu[0], (double)x[1] - (double)pu[1], (double)x[2] - (double)pu[2]};
        const double tt = ((xr[0] * dl[0] + xr[1] * dl[1]) + xr[2] * dl[2]) / ((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]);
        const float t = (float)(tt > 0.0 ? (tt < 1.0 ? tt : 1.0) : 0.0);                                    // a NaN counts as 0
        float c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float cu = colors[3 * (long long)u + a], cv = colors[3 * (long long)v + a];
            c[a] = cu + t * (cv - cu);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) colors[3 * (long long)s + a] = c[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[3 * (long long)s + a] = x[a];
#pragma unroll
    for (int k = 0; k < DEC_ROW; ++k) rows[(long long)s * DEC_ROW + k] = sum[k];
    if (!(lu || lv)) moved[s] = 1;
    vmap[d] = s;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_reindex_kernel(long long n_faces, int* __restrict__ faces, long long n_vertices,
                                                                  const int* __restrict__ vmap, unsigned char* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= n_faces) return;
    int g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int id = faces[3 * i + c];
        g[c] = dec_in(id, n_vertices) ? vmap[id] : id;                                                      // index guard: such an id stays as it is
        faces[3 * i + c] = g[c];
    }
    keep[i] = g[0] != g[1] && g[1] != g[2] && g[2] != g[0];
}

// ---- hole filling (mesh_ops.hip: dgs_fill_rank, dgs_fill_rim, dgs_fill_emit) --------------------------------------------------------
// include/dgs_mesh_ops.h states every step; dgs_amd/mesh_fill.py states the same arithmetic in PyTorch.  The ranks are integers, the
// sums of a loop are int64 fixed-point sums (exact in any order, combined on chip by simp_combine: neighbouring rim slots share a
// loop), and everything fp64 below is written operation by operation (-ffp-contract=off).
// SHAPE.  A thread per boundary half-edge (ranks), per rim slot (sums, smoothed rim), per new vertex or per new face (emission), over
// arrays in rank order: a loop's slots, vertices and faces are contiguous, so a wave reads a few rows of the loop and ring tables
// and neighbouring rows of S.  No kernel waits for another workgroup and no loop walks a list: the only loop is the 9 taps.
// GUARDS.  Every id and offset read from a buffer is range-checked before an address is formed from it; an item that fails a check
// writes its neutral output (rank -1, zeros, the face (0, 0, 0)).  A malformed successor table gives wrong ranks, never a hang:
// the number of rounds is an argument.
constexpr int FILL_THREADS = 256, FILL_ITEMS_PER_THREAD = 1, FILL_POS_BITS = 30, FILL_NRM_BITS = 28, FILL_COL_BITS = 24;
constexpr int FILL_RING_COLS = 10, FILL_TAPS = 9, FILL_MAX_ROUNDS = 31, FILL_SUM_COLS = 9;
// columns of a row of the ring table
constexpr int FR_LOOP = 0, FR_K = 1, FR_R = 2, FR_N = 3, FR_CNT = 4, FR_VBASE = 5, FR_PCNT = 6, FR_PBASE = 7, FR_FBASE = 8, FR_NF = 9;

// The packed entry of the pointer jumping: next node << 32 | distance to it.
__global__ __launch_bounds__(FILL_THREADS) void fill_rank_init_kernel(long long n_nodes, const int* __restrict__ succ,
                                                                      const int* __restrict__ leader, unsigned long long* __restrict__ out) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const int s = succ[h], l = leader[h];
    // not ranked, a successor outside the table, or the node in front of the leader (the cut): the end of a list
    const bool end = l < 0 || !dec_in(s, n_nodes) || s == l;
    out[h] = end ? (unsigned long long)h << 32 : ((unsigned long long)(unsigned)s << 32) | 1ull;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rank_round_kernel(long long n_nodes, const unsigned long long* __restrict__ in,
                                                                       unsigned long long* __restrict__ out) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const unsigned long long e = in[h];
    const unsigned long long nx = e >> 32;
    if (nx >= (unsigned long long)n_nodes) { out[h] = e; return; }                                          // index guard (init writes no such entry)
    const unsigned long long f = in[nx];
    out[h] = (f & 0xFFFFFFFF00000000ull) | ((e + f) & 0xFFFFFFFFull);
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rank_final_kernel(long long n_nodes, const int* __restrict__ leader,
                                                                       const unsigned long long* __restrict__ in, int* __restrict__ rank) {
    const long long h = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (h >= n_nodes) return;
    const int l = leader[h];
    rank[h] = l < 0 ? -1 : ((long long)l == h ? 0 : (int)((in[h] + 1ull) & 0x7FFFFFFFull));
}

struct FillFrame { double centre[3], scale, inv_scale; };

__device__ __forceinline__ double fill_clamp01(float c) { return (double)(c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f); }       // NaN counts as 0

// the rim range [off, off + n) of loop l, or false
__device__ __forceinline__ bool fill_loop(const long long* __restrict__ offsets, int l, long long n_loops, long long n_rim, long long& off, long long& n) {
    if (!dec_in(l, n_loops)) return false;
    off = offsets[l], n = offsets[l + 1] - off;
    return off >= 0 && n >= 3 && n <= n_rim && off <= n_rim - n;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_rim_kernel(long long n_vertices, const float* __restrict__ vertices, const float* __restrict__ colors,
                                                                long long n_rim, const int* __restrict__ loop_vertices, const int* __restrict__ rim_loop,
                                                                long long n_loops, const long long* __restrict__ loop_offsets, FillFrame fr,
                                                                double* __restrict__ S, double* __restrict__ SC, long long* __restrict__ rows) {
    __shared__ SimpShared<FILL_SUM_COLS> sh;
    const long long b = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    int key = -1;
    long long v[FILL_SUM_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double s[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    if (b < n_rim) {
        const int l = rim_loop[b];
        long long off, n;
        bool ok = fill_loop(loop_offsets, l, n_loops, n_rim, off, n) && b >= off && b - off < n;
        if (ok) {
            const long long i = b - off;
            const double w[FILL_TAPS] = {1.0 / 256, 8.0 / 256, 28.0 / 256, 56.0 / 256, 70.0 / 256, 56.0 / 256, 28.0 / 256, 8.0 / 256, 1.0 / 256};
            double p0[3] = {0.0, 0.0, 0.0}, p1[3] = {0.0, 0.0, 0.0}, c0[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < FILL_TAPS; ++t) {
                const long long at = ((i + (t - 4)) % n + n) % n;
                const int r = loop_vertices[off + at];
                if (!dec_in(r, n_vertices)) { ok = false; continue; }                                       // index guard
                double p[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    p[a] = ((double)vertices[3 * (long long)r + a] - fr.centre[a]) * fr.scale;
                    s[a] = t == 0 ? w[0] * p[a] : s[a] + w[t] * p[a];
                    if (t == 4) p0[a] = p[a];
                    if (t == 5) p1[a] = p[a];
                }
                if (colors) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const double c = fill_clamp01(colors[3 * (long long)r + a]);
                        sc[a] = t == 0 ? w[0] * c : sc[a] + w[t] * c;
                        if (t == 4) c0[a] = c;
                    }
                }
            }
            if (ok) {
                key = l;
                const double pos = (double)(1 << FILL_POS_BITS), nrm = (double)(1 << FILL_NRM_BITS), col = (double)(1 << FILL_COL_BITS);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int y = (a + 1) % 3, z = (a + 2) % 3;
                    v[a] = (long long)rint(p0[a] * pos);
                    v[3 + a] = (long long)rint(((p0[y] - p1[y]) * (p0[z] + p1[z])) * nrm);                    // Newell
                    v[6 + a] = (long long)rint(c0[a] * col);
                }
            } else {
                s[0] = s[1] = s[2] = sc[0] = sc[1] = sc[2] = 0.0;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            S[3 * b + a] = s[a];
            if (SC) SC[3 * b + a] = sc[a];
        }
    }
    simp_combine<FILL_SUM_COLS, 0>(sh, key, v, n_loops, rows);
}

// What the two emission kernels share: the row of the ring table an item belongs to and the rim range of its loop.
struct FillRing { int l, k, R, cnt, vbase, pcnt, pbase, fbase, nf; long long off, n; };

__device__ __forceinline__ bool fill_ring(const int* __restrict__ rings, long long n_rings, int rid, const long long* __restrict__ loop_offsets,
                                          long long n_loops, long long n_rim, FillRing& g) {
    if (!dec_in(rid, n_rings)) return false;
    const int* row = rings + (long long)rid * FILL_RING_COLS;
    g.l = row[FR_LOOP], g.k = row[FR_K], g.R = row[FR_R], g.cnt = row[FR_CNT], g.vbase = row[FR_VBASE], g.pcnt = row[FR_PCNT];
    g.pbase = row[FR_PBASE], g.fbase = row[FR_FBASE], g.nf = row[FR_NF];
    return fill_loop(loop_offsets, g.l, n_loops, n_rim, g.off, g.n) && g.n == (long long)row[FR_N] && g.k >= 1 && g.k <= g.R;
}

__global__ __launch_bounds__(FILL_THREADS) void fill_vertex_kernel(long long n_old, long long n_new, const int* __restrict__ vert_ring,
                                                                   long long n_rings, const int* __restrict__ rings, long long n_loops,
                                                                   const long long* __restrict__ loop_offsets, long long n_rim,
                                                                   const long long* __restrict__ rows, const double* __restrict__ S,
                                                                   const double* __restrict__ SC, FillFrame fr, float* __restrict__ vertices_out,
                                                                   float* __restrict__ colors_out) {
    const long long q = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (q >= n_new) return;
    float x[3] = {0.0f, 0.0f, 0.0f}, c[3] = {0.0f, 0.0f, 0.0f};
    FillRing g = {};
    const bool ok = fill_ring(rings, n_rings, vert_ring[q], loop_offsets, n_loops, n_rim, g);
    const long long j = n_old + q - g.vbase;
    if (ok && j >= 0 && j < g.cnt) {
        const long long num = j * g.n, m = g.cnt;
        const long long i0 = (num / m) % g.n, i1 = (i0 + 1) % g.n;                                         // (j < m: num / m < n already)
        const double t = (double)(num % m) / (double)m, u = 1.0 - (double)g.k / (double)g.R;
        const double dp = (double)g.n * (double)(1 << FILL_POS_BITS), dc = (double)g.n * (double)(1 << FILL_COL_BITS);
        const long long* row = rows + (long long)g.l * SIMP_ROW;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ce = (double)row[a] / dp;
            double y = ce;
            if (g.k < g.R) {
                const double s0 = S[3 * (g.off + i0) + a], s1 = S[3 * (g.off + i1) + a];
                const double s = s0 + t * (s1 - s0);
                y = ce + u * (s - ce);
            }
            x[a] = (float)(fr.centre[a] + y * fr.inv_scale);
            if (colors_out) {
                const double cc = (double)row[6 + a] / dc;
                double z = cc;
                if (g.k < g.R) {
                    const double s0 = SC[3 * (g.off + i0) + a], s1 = SC[3 * (g.off + i1) + a];
                    const double s = s0 + t * (s1 - s0);
                    z = cc + u * (s - cc);
                }
                c[a] = (float)z;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        vertices_out[3 * (n_old + q) + a] = x[a];
        if (colors_out) colors_out[3 * (n_old + q) + a] = c[a];
    }
}

// signed area of (a, b, c) against N, twice
__device__ __forceinline__ double fill_area(const double (&a)[3], const double (&b)[3], const double (&c)[3], const double (&N)[3]) {
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    double n[3];
    dec_cross(e1, e2, n);
    return (n[0] * N[0] + n[1] * N[1]) + n[2] * N[2];
}

__global__ __launch_bounds__(FILL_THREADS) void fill_face_kernel(long long n_total, long long n_new_faces, const int* __restrict__ face_ring,
                                                                 long long n_rings, const int* __restrict__ rings, long long n_loops,
                                                                 const long long* __restrict__ loop_offsets, long long n_rim,
                                                                 const int* __restrict__ loop_vertices, const long long* __restrict__ rows,
                                                                 const float* __restrict__ vertices_out, int* __restrict__ faces_out) {
    const long long f = (long long)blockIdx.x * FILL_THREADS + threadIdx.x;
    if (f >= n_new_faces) return;
    int o[3] = {0, 0, 0};
    FillRing g = {};
    const bool ok = fill_ring(rings, n_rings, face_ring[f], loop_offsets, n_loops, n_rim, g);
    const long long e = f - g.fbase;
    if (ok && e >= 0 && e < g.nf) {
        const long long n = g.n, m = g.pcnt, mi = g.cnt;
        // vertex i of the ring outside this strip: the rim (through loop_vertices) or the ring before
        auto prev = [&](long long i) { return g.pbase < 0 ? loop_vertices[g.off + i] : (int)(g.pbase + i); };
        if (n == 3 && g.nf == 1) {
            o[0] = loop_vertices[g.off], o[1] = loop_vertices[g.off + 1], o[2] = loop_vertices[g.off + 2];
        } else if (g.k == g.R) {                                                                            // the fan to the centre
            if (m >= 1 && (g.pbase >= 0 || m == n) && e < m) o[0] = prev(e), o[1] = prev((e + 1) % m), o[2] = g.vbase;
        } else if (g.k == 1) {                                                                              // rim -> ring 1: a quad per rim edge
            const long long i = e >> 1, i1 = (i + 1) % n;
            if (g.pbase < 0 && mi == n && i < n) {
                const int id[4] = {loop_vertices[g.off + i], loop_vertices[g.off + i1], (int)(g.vbase + i1), (int)(g.vbase + i)};   // r0 r1 q1 q0
                if (dec_in(id[0], n_total) && dec_in(id[1], n_total) && dec_in(id[2], n_total) && dec_in(id[3], n_total)) {
                    double p[4][3], N[3];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int a = 0; a < 3; ++a) p[c][a] = (double)vertices_out[3 * (long long)id[c] + a];
#pragma unroll
                    for (int a = 0; a < 3; ++a) N[a] = (double)rows[(long long)g.l * SIMP_ROW + 3 + a];
                    const double t1 = fill_area(p[0], p[1], p[2], N), t2 = fill_area(p[0], p[2], p[3], N);          // diagonal r0 - q1
                    const double u1 = fill_area(p[0], p[1], p[3], N), u2 = fill_area(p[1], p[2], p[3], N);          // diagonal r1 - q0
                    const double first = t1 < t2 ? t1 : t2, second = u1 < u2 ? u1 : u2;
                    if (second > first) {
                        if (e & 1) o[0] = id[1], o[1] = id[2], o[2] = id[3];
                        else o[0] = id[0], o[1] = id[1], o[2] = id[3];
                    } else {
                        if (e & 1) o[0] = id[0], o[1] = id[2], o[2] = id[3];
                        else o[0] = id[0], o[1] = id[1], o[2] = id[2];
                    }
                }
            }
        } else if (g.pbase >= 0 && m >= 1 && mi >= 1) {                                                     // ring k - 1 (m) -> ring k (mi): the merge by parameter
            if (e < m) {
                o[0] = (int)(g.pbase + e), o[1] = (int)(g.pbase + (e + 1) % m), o[2] = (int)(g.vbase + (((e + 1) * mi - 1) / m) % mi);
            } else if (e - m < mi) {
                const long long j = e - m;
                o[0] = (int)(g.pbase + (((j + 1) * m) / mi) % m), o[1] = (int)(g.vbase + (j + 1) % mi), o[2] = (int)(g.vbase + j);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) faces_out[3 * f + a] = o[a];
}

}  // namespace
