// mesh_common.h -- what more than one family header of the mesh library shares (mesh_ops.hip).  A helper lives here when two
// families use it, under a name that belongs to neither.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// ---- ids and rows ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_range(int id, long long n) { return id >= 0 && (long long)id < n; }

// the row [b, e) of a CSR table, clamped to [0, n_entries]
__device__ __forceinline__ void csr_row(const long long* __restrict__ offsets, long long i, long long n_entries, long long& b, long long& e) {
    b = offsets[i], e = offsets[i + 1];
    b = b < 0 ? 0 : (b > n_entries ? n_entries : b);
    e = e < b ? b : (e > n_entries ? n_entries : e);
}

// ---- small geometry -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&n)[3]) {
    n[0] = a[1] * b[2] - a[2] * b[1], n[1] = a[2] * b[0] - a[0] * b[2], n[2] = a[0] * b[1] - a[1] * b[0];
}

// n = (p1 - p0) x (p2 - p0) in fp32 -> its length, through the fp64 square root, which is correctly rounded on the device and in
// the PyTorch statements alike (sqrtf is not on the device)
__device__ __forceinline__ float face_normal(const float (&p)[3][3], float (&n)[3]) {
    const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
    n[0] = uy * vz - uz * vy, n[1] = uz * vx - ux * vz, n[2] = ux * vy - uy * vx;
    return (float)sqrt((double)((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]));
}

// ---- plane quadrics -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long fixed_round(float x) { return (long long)rintf(x); }
__device__ __forceinline__ long long fixed_round(double x) { return (long long)rint(x); }

// v[0..5] = the upper triangle (xx xy xz yy yz zz) of w n n^T, v[6..8] = wd n, times scale (a power of two) and rounded in T
template <class T, int N>
__device__ __forceinline__ void quadric_fixed(T w, T wd, const T (&n)[3], T scale, long long (&v)[N]) {
    static_assert(N >= 9, "six entries of A and three of b");
    int o = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) v[o++] = fixed_round(((w * n[a]) * n[b]) * scale);
#pragma unroll
    for (int a = 0; a < 3; ++a) v[6 + a] = fixed_round((wd * n[a]) * scale);
}

// The regularised system of include/dgs_mesh_ops.h, operation by operation: (A + reg I) y = reg anchor - b with reg = t 2^LAMBDA_EXP
// and t the trace of A (xx xy xz yy yz zz), solved by cofactors.  The caller accepts y only if t > 0, det is positive and finite and
// y passes its own distance test; a NaN fails every one of them.
constexpr int QUADRIC_LAMBDA_EXP = -10;

__device__ __forceinline__ void quadric_solve(const double (&A)[6], const double (&b)[3], const double (&anchor)[3], double& t, double& det,
                                              double (&y)[3]) {
    const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
    t = (a00 + a11) + a22;
    const double reg = t * 0x1p-10;
    static_assert(QUADRIC_LAMBDA_EXP == -10, "reg above is t * 2^QUADRIC_LAMBDA_EXP");
    const double m00 = a00 + reg, m11 = a11 + reg, m22 = a22 + reg;
    const double r0 = reg * anchor[0] - b[0], r1 = reg * anchor[1] - b[1], r2 = reg * anchor[2] - b[2];
    const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
    const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
    det = (m00 * c00 + a01 * c01) + a02 * c02;
    y[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    y[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    y[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
}

// ---- on-chip run combining of int64 rows ----------------------------------------------------------------------------------------
// A workgroup of SUM_THREADS items adds NCOL int64 values each to rows of SUM_ROW int64 (128 contiguous bytes) picked by a key.  It
// (1) stores key and values of its items in LDS, (2) finds the runs of equal neighbouring keys (a head is an item whose left
// neighbour has another key; ballot + popcount number the heads, a 4-entry table joins the waves), (3) gives every run to 16 lanes,
// one per column, each of which sums its column over the run out of LDS and issues ONE atomic: a wave instruction covers four runs,
// each lane group a contiguous piece of one row.  Zero sums are not sent.  Int64 additions are exact, so the grouping cannot change
// a bit.  A key outside [0, n_rows) takes part in every barrier and is skipped at the atomic: no address is formed from it.
constexpr int SUM_THREADS = 256, SUM_ROW = 16, SUM_WAVES = SUM_THREADS / 64;

template <int NCOL>
struct SumShared {
    long long val[SUM_THREADS][NCOL];
    int key[SUM_THREADS];
    int start[SUM_THREADS + 1];        // first item of every run, then SUM_THREADS
    int wave_runs[SUM_WAVES];
};

// Every thread of the workgroup calls this (no early exit before it).  COL0: the first of the NCOL columns these values go to.
template <int NCOL, int COL0>
__device__ __forceinline__ void sum_combine(SumShared<NCOL>& sh, int key, const long long (&v)[NCOL], long long n_rows,
                                            long long* __restrict__ rows) {
    static_assert(COL0 + NCOL <= SUM_ROW, "the columns lie inside a row");
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
    for (int w = 0; w < SUM_WAVES; ++w) {
        const int n = sh.wave_runs[w];
        base += w < wave ? n : 0;
        total += n;
    }
    if (head) sh.start[base + __popcll(heads & ((1ull << lane) - 1ull))] = t;
    if (t == 0) sh.start[total] = SUM_THREADS;
    __syncthreads();
    const int col = t & (SUM_ROW - 1);
    for (int r = t / SUM_ROW; r < total; r += SUM_THREADS / SUM_ROW) {
        const int s = sh.start[r], e = sh.start[r + 1], k = sh.key[s];
        if (col >= NCOL || k < 0 || k >= n_rows) continue;              // index guard: rows[k] exists
        long long sum = 0;
        for (int i = s; i < e; ++i) sum += sh.val[i][col];
        if (sum != 0) atomicAdd((unsigned long long*)(rows + (long long)k * SUM_ROW + COL0 + col), (unsigned long long)sum);
    }
    __syncthreads();                                                    // the buffers are free for the next call
}

}  // namespace
