// knn_kernels.h -- K nearest control nodes of every surfel (train_ops.hip; replaces pytorch3d.ops.knn_points for the
// control-node lookup, utils/time_utils.py:950), K <= 4, D <= 16.
//   knn_kernel: brute force.  Nodes are staged in LDS 1024 at a time, a thread keeps the K best of two query points in registers.
//   knn_refine_kernel: exact answer again from last step's indices; the seed bounds the search, 32-node blocks are culled by
//     their 3-D bounding boxes.
//   knn_refine_mfma_kernel: the same with a dense full-distance filter on the matrix cores (split bf16 operands).
// Contract of all three: every stored index is in [0, M), whatever the inputs hold, and the three agree bit for bit.  A slot that
// no node fills -- all distances of the point are NaN or infinite (a non-finite coordinate, or a point so far out that the squares
// overflow) -- holds index 0 (and dist2 = inf in the plain scan).  The result feeds the skinning kernels' gathers unchecked.
// Each kernel has its launch_* templates behind it; dispatch_K turns the run-time K into the template argument.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "train_common.h"

namespace {

// ---- KNN ------------------------------------------------------------------------------------------------------
constexpr int kKnnChunk = 1024;  // nodes staged per pass
constexpr int kKnnDpad = 16;

// Q = number of float4 per (zero-padded) node row: D <= 4*Q.  Compile-time so that the distance loop fully
// unrolls and the wave-uniform node reads become ds_read_b128 broadcasts.  Every thread owns kKnnPts query points:
// one set of LDS reads feeds kKnnPts independent distance chains (the loop is latency-, not throughput-bound).
constexpr int kKnnPts = 2;
constexpr int kKnnGrp = 4;

template <int K, int Q>
__global__ void __launch_bounds__(256) knn_kernel(int N, int M, int D, const float* __restrict__ x, const float* __restrict__ nodes,
                                                  long long* __restrict__ idx, float* __restrict__ dist2,
                                                  const float* __restrict__ x2, int D1, int stride2)
{
    __shared__ float4 s_nodes[kKnnChunk * Q];
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * kKnnPts;
    float xv[kKnnPts][4 * Q];
#pragma unroll
    for (int u = 0; u < kKnnPts; u++)
#pragma unroll
        for (int d = 0; d < 4 * Q; d++) {
            // coordinates [0, D1) come from x (row stride D1), [D1, D) from x2 (row stride stride2); x2 == nullptr: D1 = D
            float v = 0.f;
            if (p0 + u < N && d < D) v = d < D1 ? x[(size_t)(p0 + u) * D1 + d] : x2[(size_t)(p0 + u) * stride2 + d - D1];
            xv[u][d] = v;
        }
    float bd[kKnnPts][K];
    int bi[kKnnPts][K];
#pragma unroll
    for (int u = 0; u < kKnnPts; u++)
#pragma unroll
        for (int k = 0; k < K; k++) { bd[u][k] = INFINITY; bi[u][k] = 0; }
    for (int base = 0; base < M; base += kKnnChunk) {
        const int cnt = (M - base) < kKnnChunk ? (M - base) : kKnnChunk;
        __syncthreads();
        // one node row per thread and pass, every load of the pass issued before the first LDS store (a flat
        // element-wise copy is a chain of dependent global-load latencies and used to cost more than the scan)
        for (int r0 = 0; r0 < cnt; r0 += 1024) {
            float v[4][4 * Q];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = r0 + i * 256 + threadIdx.x;
#pragma unroll
                for (int d = 0; d < 4 * Q; d++) v[i][d] = (r < cnt && d < D) ? nodes[(size_t)(base + r) * D + d] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = r0 + i * 256 + threadIdx.x;
                if (r < cnt)
#pragma unroll
                    for (int q = 0; q < Q; q++) s_nodes[r * Q + q] = make_float4(v[i][4 * q], v[i][4 * q + 1], v[i][4 * q + 2], v[i][4 * q + 3]);
            }
        }
        __syncthreads();
        // groups of kKnnGrp nodes: all LDS reads of a group are issued before the first use, the kKnnPts x kKnnGrp
        // distances are independent FMA chains, and the (rare) insertions come last
        for (int j0 = 0; j0 < cnt; j0 += kKnnGrp) {
            float4 nd[kKnnGrp][Q];
#pragma unroll
            for (int g = 0; g < kKnnGrp; g++)
#pragma unroll
                for (int q = 0; q < Q; q++) nd[g][q] = s_nodes[min(j0 + g, cnt - 1) * Q + q];  // wave-uniform: LDS broadcast
            // (A v_pk_add_f32 / v_pk_fma_f32 formulation pairing the two points was measured at the same 0.23 ms: packed
            // fp32 does not issue faster than two scalar ops on gfx950 and needs extra moves to splat the node value.)
            float acc[kKnnPts][kKnnGrp];
#pragma unroll
            for (int u = 0; u < kKnnPts; u++)
#pragma unroll
                for (int g = 0; g < kKnnGrp; g++) {
                    float a = 0.f;
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        float t;
                        t = xv[u][4 * q + 0] - nd[g][q].x; a += t * t;
                        t = xv[u][4 * q + 1] - nd[g][q].y; a += t * t;
                        t = xv[u][4 * q + 2] - nd[g][q].z; a += t * t;
                        t = xv[u][4 * q + 3] - nd[g][q].w; a += t * t;
                    }
                    acc[u][g] = (j0 + g < cnt) ? a : INFINITY;
                }
#pragma unroll
            for (int u = 0; u < kKnnPts; u++) {
                float best = acc[u][0];
#pragma unroll
                for (int g = 1; g < kKnnGrp; g++) best = fminf(best, acc[u][g]);
                if (best < bd[u][K - 1]) {
#pragma unroll
                    for (int g = 0; g < kKnnGrp; g++) {
                        // insertion into the sorted K best; strict < keeps the lower index on ties
                        if (acc[u][g] < bd[u][K - 1]) {
                            bd[u][K - 1] = acc[u][g]; bi[u][K - 1] = base + j0 + g;
#pragma unroll
                            for (int k = K - 1; k > 0; k--) {
                                if (bd[u][k] < bd[u][k - 1]) {
                                    const float td = bd[u][k]; bd[u][k] = bd[u][k - 1]; bd[u][k - 1] = td;
                                    const int ti = bi[u][k]; bi[u][k] = bi[u][k - 1]; bi[u][k - 1] = ti;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kKnnPts; u++)
        if (p0 + u < N) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                idx[(size_t)(p0 + u) * K + k] = bi[u][k];
                if (dist2) dist2[(size_t)(p0 + u) * K + k] = bd[u][k];
            }
        }
}

template <int K, int Q>
int launch_knn_q(int N, int M, int D, const float* x, const float* nodes, long long* idx, float* dist2, hipStream_t s,
                 const float* x2, int D1, int stride2)
{
    const int per_block = 256 * kKnnPts;
    hipLaunchKernelGGL((knn_kernel<K, Q>), dim3((N + per_block - 1) / per_block), dim3(256), 0, s, N, M, D, x, nodes, idx, dist2,
                       x2, D1, stride2);
    return launched("knn_kernel");
}

template <int K>
int launch_knn(int N, int M, int D, const float* x, const float* nodes, long long* idx, float* dist2, hipStream_t s,
               const float* x2 = nullptr, int D1 = -1, int stride2 = 0)
{
    if (!x2) D1 = D;
    switch ((D + 3) / 4) {
    case 1: return launch_knn_q<K, 1>(N, M, D, x, nodes, idx, dist2, s, x2, D1, stride2);
    case 2: return launch_knn_q<K, 2>(N, M, D, x, nodes, idx, dist2, s, x2, D1, stride2);
    case 3: return launch_knn_q<K, 3>(N, M, D, x, nodes, idx, dist2, s, x2, D1, stride2);
    default: return launch_knn_q<K, 4>(N, M, D, x, nodes, idx, dist2, s, x2, D1, stride2);
    }
}

// ---- KNN refinement -----------------------------------------------------------------------------------------------
// Exact K nearest neighbours again, but seeded with a previous answer (last step's indices: surfels and nodes move by
// ~1e-6 per step).  The K seed nodes give an upper bound T on the K-th smallest distance; the 3-D part of the distance
// (coordinates 0..2 of D) is a lower bound of the full one, so only nodes with d3 <= T can be in the answer.  The scan
// over all M nodes therefore needs 3 of the D coordinates (7 instead of 2*D VALU operations per node) and just records
// the few candidates; full distances are evaluated for those only.  Any seed (stale, random, duplicated) gives the exact
// result: a bad seed only makes T large, a full candidate list falls back to the plain scan for that point.
//
// The scan skips whole 32-node blocks: every block has a bounding box (built next to the staged nodes), every wave the box of
// its points' search spheres (centre x, radius sqrt(T)); a block whose box misses the wave's cannot hold a candidate of any
// lane, and the test is one lane per block + one ballot.  Pays when both sides are spatially coherent -- surfels stored in the
// order of their nearest node and nodes stored along a space-filling curve (Trainer.sort_surfels / sort_nodes: 32 blocks ->
// ~4 per wave at 200 k surfels / 1024 nodes); any order gives the same, exact result.
constexpr int kKnnCap = 12;
// 512 threads x 1 point: 200k points are 3125 waves (3 per SIMD) instead of the 1563 of 256 threads x 2 points, and the node
// table (48 KB) is shared by twice the points per workgroup, so two workgroups still fit a CU.
constexpr int kRefThreads = 512;
constexpr int kRefPts = 1;
constexpr int kRefGrp = 4;   // nodes per group of LDS broadcasts in flight (8: no change)

template <int K, int Q>
__global__ void __launch_bounds__(kRefThreads) knn_refine_kernel(int N, int M, int D, const float* __restrict__ x, const float* __restrict__ nodes,
                                                         long long* __restrict__ idx, const float* __restrict__ x2, int D1, int stride2)
{
    extern __shared__ float4 s_dyn[];
    const int Mp = (M + 31) & ~31;                                        // rows padded to the 32-node scan blocks (zeros, masked)
    const int nblk = Mp >> 5;
    float4* s_nodes = s_dyn;                                              // [Mp][Q]
    float4* s_box = s_dyn + (size_t)Mp * Q;                               // [nblk][2]: min, max of the block's nodes (coordinates 0..2)
    int* s_list = reinterpret_cast<int*>(s_box + 2 * nblk);               // [kRefThreads * kRefPts][kKnnCap]
    // node table -> LDS rows of 4 Q floats (zero padded).  The table is read as a flat stream of 16-byte vectors (a 4-byte load
    // occupies the address unit as long as a 16-byte one: 24 loads per thread became 6) and scattered into the padded rows
    {
        float* s_f = reinterpret_cast<float*>(s_nodes);
        const int F = M * D, nvec = (reinterpret_cast<size_t>(nodes) & 15) == 0 ? F >> 2 : 0;
        for (int r = threadIdx.x; r < Mp; r += kRefThreads)
            for (int c = (r < M ? D : 0); c < 4 * Q; c++) s_f[r * 4 * Q + c] = 0.f;
        for (int base = 0; base < nvec; base += 8 * kRefThreads) {
            float4 q[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int v = base + i * kRefThreads + threadIdx.x;
                q[i] = v < nvec ? reinterpret_cast<const float4*>(nodes)[v] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int v = base + i * kRefThreads + threadIdx.x;
                if (v >= nvec) continue;
                int r = (4 * v) / D, c = 4 * v - r * D;
                const float e[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    s_f[r * 4 * Q + c] = e[k];
                    if (++c == D) { c = 0; r++; }
                }
            }
        }
        for (int e = 4 * nvec + threadIdx.x; e < F; e += kRefThreads) {   // the last F % 4 elements, or all of an unaligned table
            const int r = e / D, c = e - r * D;
            s_f[r * 4 * Q + c] = nodes[e];
        }
    }
    __syncthreads();
    // bounding boxes of the 32-node blocks: 16 lanes per block, two nodes each, min / max over the row of 16 with DPP shifts
    // (32 threads walking 32 nodes each left the other 480 waiting at the barrier)
    for (int b = threadIdx.x >> 4; b < nblk; b += kRefThreads >> 4) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = b * 32 + 2 * (threadIdx.x & 15) + h;
            if (j < M) {
                const float4 nd = s_nodes[j * Q];
                lo[0] = fminf(lo[0], nd.x); lo[1] = fminf(lo[1], nd.y); lo[2] = fminf(lo[2], nd.z);
                hi[0] = fmaxf(hi[0], nd.x); hi[1] = fmaxf(hi[1], nd.y); hi[2] = fmaxf(hi[2], nd.z);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
#define KNN_ROW_STEP(n)                                                                                                                         \
            lo[c] = fminf(lo[c], __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lo[c]), __builtin_bit_cast(int, lo[c]), \
                                                                                       0x110 + (n), 0xf, 0xf, false)));                         \
            hi[c] = fmaxf(hi[c], __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, hi[c]), __builtin_bit_cast(int, hi[c]), \
                                                                                       0x110 + (n), 0xf, 0xf, false)))
            KNN_ROW_STEP(1); KNN_ROW_STEP(2); KNN_ROW_STEP(4); KNN_ROW_STEP(8);
#undef KNN_ROW_STEP
        }
        if ((threadIdx.x & 15) == 15) {
            s_box[2 * b] = make_float4(lo[0], lo[1], lo[2], 0.f);
            s_box[2 * b + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
        }
    }
    __syncthreads();
    const int p0 = (blockIdx.x * kRefThreads + threadIdx.x) * kRefPts;
    float xv[kRefPts][4 * Q];
    float T[kRefPts];
    int cnt[kRefPts];
    auto full_dist = [&](int u, int j) {
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const float4 nd = s_nodes[j * Q + q];
            float t;
            t = xv[u][4 * q + 0] - nd.x; a += t * t;
            t = xv[u][4 * q + 1] - nd.y; a += t * t;
            t = xv[u][4 * q + 2] - nd.z; a += t * t;
            t = xv[u][4 * q + 3] - nd.w; a += t * t;
        }
        return a;
    };
#pragma unroll
    for (int u = 0; u < kRefPts; u++) {
        const bool in = p0 + u < N;
#pragma unroll
        for (int d = 0; d < 4 * Q; d++) {
            float v = 0.f;
            if (in && d < D) v = d < D1 ? x[(size_t)(p0 + u) * D1 + d] : x2[(size_t)(p0 + u) * stride2 + d - D1];
            xv[u][d] = v;
        }
        // bound from the seed (K distinct valid nodes), slightly inflated never hurts: it is only a filter
        int sj[K];
        bool ok = in;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const long long j = in ? idx[(size_t)(p0 + u) * K + k] : 0;
            ok = ok && j >= 0 && j < M;
            sj[k] = (int)(j < 0 ? 0 : (j >= M ? M - 1 : j));
        }
#pragma unroll
        for (int k = 1; k < K; k++)
#pragma unroll
            for (int k2 = 0; k2 < k; k2++) ok = ok && sj[k] != sj[k2];
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) t = fmaxf(t, full_dist(u, sj[k]));
        T[u] = in ? (ok ? t : INFINITY) : -1.f;
        cnt[u] = 0;
    }
    // ---- scan: 3-D lower bound only.  Branch-free inner loop: the sign of d3 - T' is shifted into a 32-node hit word
    // (v_alignbit), 7 VALU operations per (node, point); the words are drained once per 32 nodes.
    float Tn[kRefPts];
#pragma unroll
    for (int u = 0; u < kRefPts; u++) Tn[u] = -(T[u] * (1.0f + 1e-6f) + 1e-30f);   // inflated: d3 == T must stay a hit
    // box of the wave's search spheres (lanes past N have T = -1: no sphere).  |x_c - n_c| <= sqrt(d3) <= sqrt(-Tn) on every axis
    // for a hit; the radius is rounded up generously, the box only filters
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int u = 0; u < kRefPts; u++)
        if (T[u] >= 0.f) {
            const float r = sqrtf(-Tn[u]) * 1.0001f + 1e-30f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                blo[c] = fminf(blo[c], xv[u][c] - r);
                bhi[c] = fmaxf(bhi[c], xv[u][c] + r);
            }
        }
    // FOUR boxes per wave, one per 16 lanes: where consecutive points change their nearest node across a jump of the node order,
    // one box over all 64 lanes spans the jump and touches most of the blocks (mean 8 of 32 but up to 23: those waves set the
    // kernel's time); the union of four tight boxes does not
    // min / max over each row of 16 lanes with DPP row shifts (lane 15 of a row ends up with the row's result; a lane without a
    // source keeps its own value), then the four results to scalar registers: no LDS traffic (48 ds_bpermute before)
    const int lane = threadIdx.x & 63;
    float qlo[4][3], qhi[4][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float lo = blo[c], hi = bhi[c];
#define KNN_ROW_STEP(n)                                                                                                                   \
        lo = fminf(lo, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, lo), __builtin_bit_cast(int, lo),   \
                                                                             0x110 + (n), 0xf, 0xf, false)));                             \
        hi = fmaxf(hi, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, hi), __builtin_bit_cast(int, hi),   \
                                                                             0x110 + (n), 0xf, 0xf, false)))
        KNN_ROW_STEP(1); KNN_ROW_STEP(2); KNN_ROW_STEP(4); KNN_ROW_STEP(8);
#undef KNN_ROW_STEP
#pragma unroll
        for (int q = 0; q < 4; q++) {
            qlo[q][c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo), 16 * q + 15));
            qhi[q][c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hi), 16 * q + 15));
        }
    }
    for (int bb = 0; bb < nblk; bb += 64) {
    bool touch = false;
    if (bb + lane < nblk) {
        const float4 lo = s_box[2 * (bb + lane)], hi = s_box[2 * (bb + lane) + 1];
#pragma unroll
        for (int q = 0; q < 4; q++)
            touch = touch || (lo.x <= qhi[q][0] && hi.x >= qlo[q][0] && lo.y <= qhi[q][1] && hi.y >= qlo[q][1] && lo.z <= qhi[q][2] &&
                              hi.z >= qlo[q][2]);
    }
    unsigned long long blocks = __ballot(touch);
    while (blocks) {
        const int j0 = (bb + __builtin_ctzll(blocks)) * 32;
        blocks &= blocks - 1;
        // ONE LDS read per block: lane g fetches node j0 + g (a wave-wide broadcast read of a node occupies the LDS pipe like any
        // other 1-KB read, and 32 of them per block were what bounded the scan: 28 us whatever the instruction count).  Lane g also
        // tests its node against the wave's boxes once for all lanes; the survivors (a third of a touched block) go to scalar
        // registers (v_readlane) and are tested per point
        float4 mine = make_float4(0.f, 0.f, 0.f, 0.f);
        bool inb = false;
        if (lane < 32 && j0 + lane < M) {
            mine = s_nodes[(j0 + lane) * Q];
#pragma unroll
            for (int q = 0; q < 4; q++)
                inb = inb || (mine.x >= qlo[q][0] && mine.x <= qhi[q][0] && mine.y >= qlo[q][1] && mine.y <= qhi[q][1] &&
                              mine.z >= qlo[q][2] && mine.z <= qhi[q][2]);
        }
        const unsigned sv = (unsigned)__ballot(inb);   // bit g <-> node j0 + g
        if (sv == 0u) continue;
        for (unsigned m = sv; m; m &= m - 1) {
            const int g = __builtin_ctz(m);
            const float nx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.x), g));
            const float ny = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.y), g));
            const float nz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.z), g));
#pragma unroll
            for (int u = 0; u < kRefPts; u++) {
                float t, a;
                t = xv[u][0] - nx; a = fmaf(t, t, Tn[u]);
                t = xv[u][1] - ny; a = fmaf(t, t, a);
                t = xv[u][2] - nz; a = fmaf(t, t, a);
                if (a < 0.f) {   // a candidate of this point (3 per point on average: the branch is skipped by most waves)
                    if (cnt[u] < kKnnCap) s_list[(threadIdx.x * kRefPts + u) * kKnnCap + cnt[u]] = j0 + g;
                    cnt[u]++;
                }
            }
        }
    }
    }
    // ---- candidates (ascending index, strict < on insertion: ties keep the lower index like the plain scan)
#pragma unroll
    for (int u = 0; u < kRefPts; u++) {
        if (p0 + u >= N) continue;
        float bd[K];
        int bi[K];
#pragma unroll
        for (int k = 0; k < K; k++) { bd[k] = INFINITY; bi[k] = 0; }
        const bool listed = cnt[u] <= kKnnCap;
        const int n = listed ? cnt[u] : M;
        for (int c = 0; c < n; c++) {
            const int j = listed ? s_list[(threadIdx.x * kRefPts + u) * kKnnCap + c] : c;
            const float dj = full_dist(u, j);
            if (dj < bd[K - 1]) {
                bd[K - 1] = dj; bi[K - 1] = j;
#pragma unroll
                for (int k = K - 1; k > 0; k--) {
                    if (bd[k] < bd[k - 1]) {
                        const float td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td;
                        const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < K; k++) idx[(size_t)(p0 + u) * K + k] = bi[k];
    }
}

template <int K, int Q>
int launch_knn_refine_q(int N, int M, int D, const float* x, const float* nodes, long long* idx, hipStream_t s, const float* x2, int D1,
                        int stride2)
{
    const int per_block = kRefThreads * kRefPts;
    const size_t lds = (size_t)((M + 31) & ~31) * Q * sizeof(float4) + (size_t)((M + 31) >> 5) * 2 * sizeof(float4) +
                       (size_t)kRefThreads * kRefPts * kKnnCap * sizeof(int);
    hipLaunchKernelGGL((knn_refine_kernel<K, Q>), dim3((N + per_block - 1) / per_block), dim3(kRefThreads), lds, s, N, M, D, x, nodes, idx, x2, D1,
                       stride2);
    return launched("knn_refine_kernel");
}

// ---- seeded refine on the matrix cores ---------------------------------------------------------------------------------
// The 3-D block / box culling of knn_refine_kernel needs the K-th seed distance to be a SPATIAL radius.  In a trained scene it is
// not: the 8 hyper coordinates of surfels and nodes drift apart, the 11-D distance of the third neighbour exceeds the node spacing
// several times, every block is touched, candidate lists overflow, and the kernel is slower than the plain scan (172 us at 125 k
// surfels x 512 nodes against 36 us on the untrained scene).  This kernel filters with the FULL distance instead, dense and
// data-independent:   score[j][i] = |n_j|^2 - 2 x_i . n_j  (= d^2 - |x_i|^2)  for 32 nodes x 32 points per matrix instruction.
//   * f32-input MFMA runs at the vector rate on gfx950 (64 cycles per 32x32x2), bf16 MFMA sixteen times faster, so both operands
//     are split  v = hi + lo  (two bf16, 16 mantissa bits) and  x.n ~ xh.nh + xh.nl + xl.nh : three v_mfma_f32_32x32x16_bf16 per
//     tile (K = 16 slots: 11 coordinates, |n|^2 as hi + lo against 1, 3 spare) instead of six f32 ones at four times the cycles
//     each.  What is dropped (xl.nl and the rounding of the lo parts) is below 1.2e-5 (|x|^2 + |n|^2); products are exact in the
//     f32 accumulator.  This is only the FILTER: a node is a candidate of point i when  score <= T_i - |x_i|^2 + eps,  T_i the
//     exact distance of the K-th seed neighbour, eps = 1e-4 (|x|^2 + max |n|^2), so no node within the seed's bound is missed.
//   * the accumulator starts at -(threshold), a hit is a SIGN BIT, and the 16 results of a tile are shifted into a per-lane hit
//     word with one v_alignbit_b32 each: no compare, no branch, no list in LDS.
//   * the K plus few candidates are evaluated exactly (f32 differences, the same operation order as the plain scan) and ranked
//     (distance, then index).  Two lanes (l, l + 32) share a point and own alternating groups of 4 rows of every 32-node tile (the
//     D layout of the instruction); their top-K lists are merged at the end.  A garbage seed (T = inf) sets every bit: that lane
//     scans its rows itself.
constexpr int kRmThreads = 512;   // 8 waves x 32 points
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned bf16_rne(float v)          // round to nearest even; inputs are finite
{
    const unsigned u = __float_as_uint(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// v -> (hi, lo) bf16 bit patterns with hi + lo ~ v to 16 mantissa bits
__device__ __forceinline__ void bf16_split(float v, unsigned& hi, unsigned& lo)
{
    hi = bf16_rne(v);
    lo = bf16_rne(v - __uint_as_float(hi << 16));
}

// TP: pairs of 32-node tiles (one 32-bit hit word per pair and lane), Mp <= 64 TP
template <int K, int TP>
__global__ void __launch_bounds__(kRmThreads) knn_refine_mfma_kernel(int N, int M, int D, const float* __restrict__ x, const float* __restrict__ nodes,
                                                                     long long* __restrict__ idx, const float* __restrict__ x2, int D1, int stride2)
{
    extern __shared__ float s_n[];                                      // [Mp][12] f32: n_0 .. n_10 (zero padded), |n|^2
    const int Mp = (M + 31) & ~31, ntiles = Mp >> 5;
    uint4* s_hi = reinterpret_cast<uint4*>(s_n + (size_t)Mp * 12);      // [Mp][2] x 8 bf16: hi parts of n_0 .. n_10, |n|^2 hi, |n|^2 lo, 0 0 0
    uint4* s_lo = s_hi + (size_t)Mp * 2;                                // [Mp][2] x 8 bf16: lo parts of n_0 .. n_10, 0 ...
    __shared__ float s_max[kRmThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    float n2max = 0.f;
    for (int j = tid; j < Mp; j += kRmThreads) {                         // one node per thread: its row's loads are all in flight at once
        float v[11];
#pragma unroll
        for (int c = 0; c < 11; c++) v[c] = (j < M && c < D) ? nodes[(size_t)j * D + c] : 0.f;
        float n2 = 0.f;
#pragma unroll
        for (int c = 0; c < 11; c++) n2 += v[c] * v[c];
        if (j < M) n2max = fmaxf(n2max, n2); else n2 = 3.0e38f;          // padded rows never qualify
        float4* row = reinterpret_cast<float4*>(s_n + (size_t)j * 12);
        row[0] = make_float4(v[0], v[1], v[2], v[3]); row[1] = make_float4(v[4], v[5], v[6], v[7]); row[2] = make_float4(v[8], v[9], v[10], n2);
        unsigned h[13], l[13];
#pragma unroll
        for (int c = 0; c < 11; c++) bf16_split(v[c], h[c], l[c]);
        bf16_split(n2, h[11], h[12]);
        s_hi[2 * j] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        s_hi[2 * j + 1] = make_uint4(h[8] | (h[9] << 16), h[10] | (h[11] << 16), h[12], 0u);
        s_lo[2 * j] = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
        s_lo[2 * j + 1] = make_uint4(l[8] | (l[9] << 16), l[10], 0u, 0u);
    }
    for (int d = 32; d >= 1; d >>= 1) n2max = fmaxf(n2max, __shfl_xor(n2max, d, 64));
    if (lane == 0) s_max[tid >> 6] = n2max;
    __syncthreads();
    n2max = s_max[0];
#pragma unroll
    for (int w = 1; w < kRmThreads / 64; w++) n2max = fmaxf(n2max, s_max[w]);

    // a wave takes groups of 32 points; the host sizes the grid so that every wave gets the same number of groups and all
    // workgroups are resident at once (782 workgroups on 768 slots ran as two rounds: twice the time)
    const int ngroups = (N + 31) >> 5, nwaves = gridDim.x * (kRmThreads / 64);
    for (int grp = blockIdx.x * (kRmThreads / 64) + (tid >> 6); grp < ngroups; grp += nwaves) {
    const int p = grp * 32 + (lane & 31);
    const bool in = p < N;
    float xv[11];
#pragma unroll
    for (int d = 0; d < 11; d++) {
        float v = 0.f;
        if (in && d < D) v = d < D1 ? x[(size_t)p * D1 + d] : x2[(size_t)p * stride2 + d - D1];
        xv[d] = v;
    }
    int sj[K];
    bool ok = in;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const long long j = in ? idx[(size_t)p * K + k] : 0;
        ok = ok && j >= 0 && j < M;
        sj[k] = (int)(j < 0 ? 0 : (j >= M ? M - 1 : j));
    }
#pragma unroll
    for (int k = 1; k < K; k++)
#pragma unroll
        for (int k2 = 0; k2 < k; k2++) ok = ok && sj[k] != sj[k2];
    auto full_dist = [&](int j) {
        const float4 n0 = *reinterpret_cast<const float4*>(s_n + j * 12), n1 = *reinterpret_cast<const float4*>(s_n + j * 12 + 4),
                     n2 = *reinterpret_cast<const float4*>(s_n + j * 12 + 8);
        float a = 0.f, t;
        // same order of operations as knn_kernel / knn_refine_kernel (groups of four coordinates): identical distances, identical ties
        t = xv[0] - n0.x; a += t * t; t = xv[1] - n0.y; a += t * t; t = xv[2] - n0.z; a += t * t; t = xv[3] - n0.w; a += t * t;
        t = xv[4] - n1.x; a += t * t; t = xv[5] - n1.y; a += t * t; t = xv[6] - n1.z; a += t * t; t = xv[7] - n1.w; a += t * t;
        t = xv[8] - n2.x; a += t * t; t = xv[9] - n2.y; a += t * t; t = xv[10] - n2.z; a += t * t;
        return a;
    };
    // bound from the seed (K distinct valid nodes): exact distance of its farthest member
    float T = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) T = fmaxf(T, full_dist(sj[k]));
    if (!ok) T = INFINITY;
    float xx = 0.f;
#pragma unroll
    for (int d = 0; d < 11; d++) xx += xv[d] * xv[d];
    // hit <=> score - thr < 0.  The subtraction rides in the accumulator: the first MFMA of a tile starts from C = -thr
    const float nthr = in ? -(T * (1.0f + 1e-6f) - xx + (1e-4f * (xx + n2max) + 1e-30f)) : INFINITY;
    f32x16 cthr;
#pragma unroll
    for (int v = 0; v < 16; v++) cthr[v] = nthr;
    // B operands of this lane's half of the K slots: slots 0..7 = coordinates 0..7 | slots 8..15 = coordinates 8..10, 1, 1, 0, 0, 0
    bf16x8 bh, bl;
    {
        unsigned h[8], l[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float v = half ? (e < 3 ? -2.0f * xv[8 + (e < 3 ? e : 0)] : 0.f) : -2.0f * xv[e];      // (no dynamic register index)
            bf16_split(v, h[e], l[e]);
        }
        if (half) { h[3] = 0x3f80u; h[4] = 0x3f80u; }                     // 1.0 against |n|^2 hi and lo
        bh = __builtin_bit_cast(bf16x8, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)));
        bl = __builtin_bit_cast(bf16x8, make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)));
    }
    unsigned hits[TP];
    const uint4* ahi = s_hi + 2 * (lane & 31) + half;
    const uint4* alo = s_lo + 2 * (lane & 31) + half;
#pragma unroll
    for (int w = 0; w < TP; w++) {
        unsigned word = 0u;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int t = 2 * w + u;
            if (t < ntiles) {                                            // wave-uniform
                const bf16x8 nh = __builtin_bit_cast(bf16x8, ahi[t * 64]), nl = __builtin_bit_cast(bf16x8, alo[t * 64]);
                f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nh, bh, cthr, 0, 0, 0);     // nh.xh + |n|^2 - thr
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nl, bh, acc, 0, 0, 0);             // nl.xh   (|n|^2 slots of nl are 0)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(nh, bl, acc, 0, 0, 0);             // nh.xl   (those slots of xl are 0)
                // the sign bits of the 16 results are shifted into the hit word, first result ends highest (v_alignbit_b32)
#pragma unroll
                for (int v = 0; v < 16; v++) word = __builtin_amdgcn_alignbit(word, __float_as_uint(acc[v]), 31);
            } else {
                word <<= 16;
            }
        }
        hits[w] = word;
    }
    // ---- exact evaluation of the candidates (ties keep the lower index like the plain scan)
    // D[i][j] of the instruction: lane = j + 32 ((i / 4) % 2), register v = 4 (i / 8) + i % 4  =>  row i = 8 (v / 4) + 4 half + v % 4;
    // bit 31 - (16 u + v) of word w is row i of tile 2 w + u
    float bd[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; k++) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
    // an infinite distance (a point with an infinite coordinate, or so far out that the square overflows) is never inserted, like
    // in the plain scan, where inf < inf is false; a NaN distance fails every comparison.  An unfilled slot keeps 0x7fffffff and
    // is stored as 0 (below): what the other two kernels' lists start with
    auto offer = [&](float dj, int j) {
        if (dj < bd[K - 1] || (dj == bd[K - 1] && dj < INFINITY && j < bi[K - 1])) {
            bd[K - 1] = dj; bi[K - 1] = j;
#pragma unroll
            for (int k = K - 1; k > 0; k--) {
                if (bd[k] < bd[k - 1] || (bd[k] == bd[k - 1] && bi[k] < bi[k - 1])) {
                    const float td = bd[k]; bd[k] = bd[k - 1]; bd[k - 1] = td;
                    const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti;
                }
            }
        }
    };
    // every trip each lane takes ITS next candidate, whichever word it is in: the number of trips is the largest candidate count of a
    // lane (5-6), not the sum over the words of the largest count per word (14 with 1.6 candidates per lane spread over 8 words)
    for (;;) {
        unsigned w = 0u;
        int wi = 0;
#pragma unroll
        for (int k = TP - 1; k >= 0; k--) { const bool nz = hits[k] != 0u; w = nz ? hits[k] : w; wi = nz ? k : wi; }
        if (__ballot(w != 0u) == 0ull) break;
        if (w != 0u) {
            const int q = __builtin_clz(w);                  // 16 u + v
            const unsigned bit = 0x80000000u >> q;
#pragma unroll
            for (int k = 0; k < TP; k++) hits[k] &= k == wi ? ~bit : ~0u;
            const int v = q & 15;
            const int j = ((2 * wi + (q >> 4)) << 5) + 8 * (v >> 2) + 4 * half + (v & 3);
            if (j < M) offer(full_dist(j), j);
        }
    }
    // merge with the partner lane's list
    float od[K];
    int oi[K];
#pragma unroll
    for (int k = 0; k < K; k++) { od[k] = __shfl_xor(bd[k], 32, 64); oi[k] = __shfl_xor(bi[k], 32, 64); }
    if (in && half == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) offer(od[k], oi[k]);
#pragma unroll
        for (int k = 0; k < K; k++) idx[(size_t)p * K + k] = bi[k] == 0x7fffffff ? 0 : bi[k];
    }
    }   // groups
}

template <int K, int TP>
int launch_knn_refine_mfma_tp(int N, int M, int D, const float* x, const float* nodes, long long* idx, hipStream_t s, const float* x2, int D1, int stride2)
{
    const int Mp = (M + 31) & ~31;
    const size_t lds = (size_t)Mp * (12 * sizeof(float) + 4 * sizeof(uint4));
    static const int cus = [] { int dev = 0, n = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
                                return n > 0 ? n : 256; }();
    const int per_cu = lds > 80 * 1024 ? 1 : 2;                                         // resident workgroups per CU (LDS: 112 B per node; VGPRs: 2)
    const int wpb = kRmThreads / 64, ngroups = (N + 31) / 32, slots = cus * per_cu * wpb;
    const int iters = (ngroups + slots - 1) / slots, waves = (ngroups + iters - 1) / iters;
    hipLaunchKernelGGL((knn_refine_mfma_kernel<K, TP>), dim3((waves + wpb - 1) / wpb), dim3(kRmThreads), lds, s, N, M, D, x, nodes, idx, x2, D1,
                       stride2);
    return launched("knn_refine_mfma_kernel");
}

template <int K>
int launch_knn_refine_mfma(int N, int M, int D, const float* x, const float* nodes, long long* idx, hipStream_t s, const float* x2, int D1, int stride2)
{
    if (M <= 256) return launch_knn_refine_mfma_tp<K, 4>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    if (M <= 512) return launch_knn_refine_mfma_tp<K, 8>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    return launch_knn_refine_mfma_tp<K, 16>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
}

template <int K>
int launch_knn_refine(int N, int M, int D, const float* x, const float* nodes, long long* idx, hipStream_t s, const float* x2, int D1,
                      int stride2, bool mfma)
{
    if (!x2) D1 = D;
    if (mfma && D <= 11 && M <= 1024) return launch_knn_refine_mfma<K>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    switch ((D + 3) / 4) {
    case 1: return launch_knn_refine_q<K, 1>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    case 2: return launch_knn_refine_q<K, 2>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    case 3: return launch_knn_refine_q<K, 3>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    default: return launch_knn_refine_q<K, 4>(N, M, D, x, nodes, idx, s, x2, D1, stride2);
    }
}

// f(std::integral_constant<int, K>) for the run-time K in 1..4 (validated by the callers; anything else takes 4)
template <class F>
int dispatch_K(int K, F&& f)
{
    switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}

}  // namespace
