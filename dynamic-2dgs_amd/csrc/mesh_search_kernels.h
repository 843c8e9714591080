// mesh_search_kernels.h -- the two all-pairs searches of the mesh metrics (mesh_ops.hip: dgs_nn_search, dgs_tri_search).  The two
// kernels share their shape and nothing else: each keeps its own statement of the query state and the packed-minimum commit.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_common.h"

namespace {

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
// A workgroup owns NN_Q = 256 x NN_K queries (each thread NN_K of them in registers: coordinates, best d2, best index) and one slice
// of the reference set, which it walks in rounds of NN_T points.  A round is staged into LDS with coalesced loads of the raw
// [n, 3] floats and de-interleaved on the way (x | y | z planes), so the inner loop reads four points with three 16-byte LDS reads
// at an address every lane shares: a broadcast, no bank conflict, and one LDS instruction per 16 / 3 query-point pairs of a
// thread.  Scanning the slice in ascending index with a strict `<` keeps the lowest index among equal distances; across slices the
// packed (d2 bits, index) minimum does.  Per pair: 3 subtractions, 3 multiplications, 2 additions, compare, 2 selects.
constexpr int NN_THREADS = 256, NN_K = 4, NN_Q = NN_THREADS * NN_K, NN_T = 1024, NN_CHUNK = 4096;

__global__ __launch_bounds__(NN_THREADS) void nn_search_kernel(long long n_query, const float* __restrict__ query, long long n_ref,
                                                               const float* __restrict__ ref, long long ref_chunk,
                                                               unsigned long long* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) float pts[3 * NN_T];
    const long long q0 = (long long)blockIdx.x * NN_Q + threadIdx.x;       // this thread's queries: q0 + k * NN_THREADS
    const long long r_begin = (long long)blockIdx.y * ref_chunk;           // the host clamps ref_chunk to n_ref: no overflow
    const long long r_end = r_begin + ref_chunk < n_ref ? r_begin + ref_chunk : n_ref;
    float qx[NN_K], qy[NN_K], qz[NN_K], bd[NN_K];
    int bi[NN_K];
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const long long q = q0 + (long long)k * NN_THREADS;
        const bool live = q < n_query;                                     // a thread past the end computes on zeros and stores nothing
        qx[k] = live ? query[3 * q] : 0.0f, qy[k] = live ? query[3 * q + 1] : 0.0f, qz[k] = live ? query[3 * q + 2] : 0.0f;
        bd[k] = __builtin_inff(), bi[k] = 0;
    }
    auto visit = [&](float x, float y, float z, int r) {
#pragma unroll
        for (int k = 0; k < NN_K; ++k) {
            const float dx = qx[k] - x, dy = qy[k] - y, dz = qz[k] - z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const bool less = d < bd[k];
            bd[k] = less ? d : bd[k], bi[k] = less ? r : bi[k];
        }
    };
    for (long long rs = r_begin; rs < r_end; rs += NN_T) {
        const int n = (int)(r_end - rs < NN_T ? r_end - rs : NN_T);       // points of this round: only they are staged and read
        __syncthreads();                                                   // the previous round's readers are done
        const float* src = ref + 3 * rs;
        for (int e = threadIdx.x; e < 3 * n; e += NN_THREADS) {            // 3 (rs + n) <= 3 n_ref: inside the reference array
            const int p = e / 3;
            pts[(e - 3 * p) * NN_T + p] = src[e];
        }
        __syncthreads();
        const int base = (int)(rs - r_begin);                              // index within the slice (< n_ref < 2^31)
        int j = 0;
        for (; j + 4 <= n; j += 4) {
            const float4 X = *reinterpret_cast<const float4*>(&pts[j]), Y = *reinterpret_cast<const float4*>(&pts[NN_T + j]),
                         Z = *reinterpret_cast<const float4*>(&pts[2 * NN_T + j]);
            visit(X.x, Y.x, Z.x, base + j), visit(X.y, Y.y, Z.y, base + j + 1);
            visit(X.z, Y.z, Z.z, base + j + 2), visit(X.w, Y.w, Z.w, base + j + 3);
        }
        for (; j < n; ++j) visit(pts[j], pts[NN_T + j], pts[2 * NN_T + j], base + j);
    }
#pragma unroll
    for (int k = 0; k < NN_K; ++k) {
        const long long q = q0 + (long long)k * NN_THREADS;
        if (q < n_query)
            atomicMin(&best[q], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)(unsigned)(r_begin + bi[k]));
    }
}

// ---- closest triangle -----------------------------------------------------------------------------------------------------------
// The shape of nn_search_kernel with a table row where that one has a point.  A workgroup owns TRI_Q = 256 x TRI_K queries (each
// thread TRI_K of them in registers: coordinates, best d2, best face) and one slice of the table, which it walks in rounds of TRI_T
// rows.  A round is a straight copy of TRI_T x 144 bytes into LDS (16-byte loads and stores, coalesced); the inner loop reads one
// row with nine 16-byte LDS reads at an address every lane shares -- a broadcast -- and evaluates it for the thread's TRI_K
// queries, 92 VALU instructions each (no fma, no division; the clamp is an output modifier of a multiply), so the LDS sees one
// instruction per 41 VALU instructions.
// Sizing: 256 rows are 36 KB, four workgroups per CU (of 160 KB) = four waves per SIMD, which is also what the registers allow
// (126 VGPRs): a broadcast row is 34 live VGPRs next to 20 of query state and the pair's temporaries.  More queries per thread
// would amortise the row further but the LDS is already idle 80 % of the time; fewer would halve the work per LDS read for nothing.
constexpr int TRI_THREADS = 256, TRI_K = 4, TRI_Q = TRI_THREADS * TRI_K, TRI_T = 256, TRI_ROW = 36, TRI_ROW4 = TRI_ROW / 4, TRI_CHUNK = 4096;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// squared distance of P to the segment from O along e, r = 1 / dot(e, e) or 0;  (wx, wy, wz) = P - O
__device__ __forceinline__ float segment_d2(float wx, float wy, float wz, float ex, float ey, float ez, float r) {
    const float t = clamp01(dot3(wx, wy, wz, ex, ey, ez) * r);
    const float cx = wx - t * ex, cy = wy - t * ey, cz = wz - t * ez;
    return dot3(cx, cy, cz, cx, cy, cz);
}

__global__ __launch_bounds__(TRI_THREADS) void tri_search_kernel(long long n_query, const float* __restrict__ query, long long n_tri,
                                                                 const float4* __restrict__ table, long long tri_chunk,
                                                                 unsigned long long* __restrict__ best) {
    __shared__ float4 rows[TRI_T * TRI_ROW4];
    const long long q0 = (long long)blockIdx.x * TRI_Q + threadIdx.x;      // this thread's queries: q0 + k * TRI_THREADS
    const long long f_begin = (long long)blockIdx.y * tri_chunk;           // the host clamps tri_chunk to n_tri: no overflow
    const long long f_end = f_begin + tri_chunk < n_tri ? f_begin + tri_chunk : n_tri;
    float qx[TRI_K], qy[TRI_K], qz[TRI_K], bd[TRI_K];
    int bi[TRI_K];
#pragma unroll
    for (int k = 0; k < TRI_K; ++k) {
        const long long q = q0 + (long long)k * TRI_THREADS;
        const bool live = q < n_query;                                     // a thread past the end computes on zeros and stores nothing
        qx[k] = live ? query[3 * q] : 0.0f, qy[k] = live ? query[3 * q + 1] : 0.0f, qz[k] = live ? query[3 * q + 2] : 0.0f;
        bd[k] = __builtin_inff(), bi[k] = 0;
    }
    for (long long fs = f_begin; fs < f_end; fs += TRI_T) {
        const int n = (int)(f_end - fs < TRI_T ? f_end - fs : TRI_T);     // rows of this round: only they are staged and read
        __syncthreads();                                                   // the previous round's readers are done
        const float4* src = table + fs * TRI_ROW4;
        for (int e = threadIdx.x; e < n * TRI_ROW4; e += TRI_THREADS)      // (fs + n) rows <= n_tri rows: inside the table;
            rows[e] = src[e];                                              // e < TRI_T * TRI_ROW4: inside the LDS array
        __syncthreads();
        const int base = (int)(fs - f_begin);                              // index within the slice (< n_tri < 2^31)
        for (int j = 0; j < n; ++j) {
            float f[TRI_ROW];
#pragma unroll
            for (int v = 0; v < TRI_ROW4; ++v) {
                const float4 x = rows[j * TRI_ROW4 + v];
                f[4 * v] = x.x, f[4 * v + 1] = x.y, f[4 * v + 2] = x.z, f[4 * v + 3] = x.w;
            }
            // A 0..2, B 3..5, C 6..8, e0 9..11, e1 12..14, e2 15..17, n 18..20, m0 21..23, m1 24..26, m2 27..29, r0 r1 r2 rn 30..33
#pragma unroll
            for (int k = 0; k < TRI_K; ++k) {
                const float ax = qx[k] - f[0], ay = qy[k] - f[1], az = qz[k] - f[2];
                const float bx = qx[k] - f[3], by = qy[k] - f[4], bz = qz[k] - f[5];
                const float cx = qx[k] - f[6], cy = qy[k] - f[7], cz = qz[k] - f[8];
                const float s0 = segment_d2(ax, ay, az, f[9], f[10], f[11], f[30]);
                const float s1 = segment_d2(bx, by, bz, f[12], f[13], f[14], f[31]);
                const float s2 = segment_d2(cx, cy, cz, f[15], f[16], f[17], f[32]);
                const float edges = fminf(fminf(s0, s1), s2);
                const bool inside = (dot3(ax, ay, az, f[21], f[22], f[23]) >= 0.0f) & (dot3(bx, by, bz, f[24], f[25], f[26]) >= 0.0f) &
                                    (dot3(cx, cy, cz, f[27], f[28], f[29]) >= 0.0f) & (f[33] > 0.0f);
                const float h = dot3(ax, ay, az, f[18], f[19], f[20]);
                const float pl = (h * h) * f[33];
                const float d = inside ? fminf(pl, edges) : edges;
                const bool less = d < bd[k];                               // strict: the lowest face among equal distances stays
                bd[k] = less ? d : bd[k], bi[k] = less ? base + j : bi[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TRI_K; ++k) {
        const long long q = q0 + (long long)k * TRI_THREADS;
        if (q < n_query)
            atomicMin(&best[q], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)(unsigned)(f_begin + bi[k]));
    }
}

}  // namespace
