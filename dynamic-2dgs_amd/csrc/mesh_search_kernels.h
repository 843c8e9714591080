// mesh_search_kernels.h -- the all-pairs searches of the mesh metrics (mesh_ops.hip: dgs_nn_search, dgs_tri_search, dgs_winding_sum
// and, at the end, the kernels of dgs_emd_auction).  The first three kernels share their shape and nothing else: each keeps its own
// statement of the query state and of its commit (a packed minimum, a packed minimum, an integer sum); the auction's bidding pass
// keeps a top-2 and is described with its kernels.
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

// ---- winding number -------------------------------------------------------------------------------------------------------------
// The shape of tri_search_kernel with a sum where that one has a minimum (dgs_winding_sum; include/dgs_mesh_ops.h states the
// quantity, dgs_amd/mesh_metrics.py: winding_sums_torch is the same statement in PyTorch).  A workgroup owns WIND_Q = 256 x WIND_K
// queries (each thread WIND_K of them in registers: coordinates and one 64-bit integer accumulator) and one slice of the table,
// which it walks in rounds of WIND_T rows.  A round is a straight copy of WIND_T x 48 bytes into LDS; the inner loop reads one row
// with three 16-byte LDS reads at an address every lane shares -- a broadcast -- and evaluates it for the thread's WIND_K queries.
// Per pair the half solid angle is turned into the integer rint(theta * 2^28) before it is added: integer addition has no order, so
// the rounds of a slice, the slices (one 64-bit atomic add per query and slice) and the PyTorch statement all give the same bits.
// Per pair: 9 subtractions, six dot products, three IEEE square roots, the 8 operations of the denominator, one IEEE division, 14
// operations of the Horner scheme and about 20 of reflections, guards and the conversion -- the ISA count is in DESIGN section 22;
// the LDS sees three instructions per WIND_K pairs and is idle.
// Sizing: 256 rows are 12 KB of LDS, which never limits; the registers do (DESIGN section 22 records the count the compiler
// reports).  The kernel is bound by VALU issue, four independent pairs per thread give the scheduler its parallelism, so
// occupancy beyond two waves per SIMD buys nothing.  WIND_CHUNK = 1024 rows per slice: a small mesh still spreads over the
// device (10^5 queries x 5000 faces are 490 workgroups), a workgroup still evaluates 2^20 pairs per 1024 atomics.
constexpr int WIND_THREADS = 256, WIND_K = 4, WIND_Q = WIND_THREADS * WIND_K, WIND_T = 256, WIND_ROW = 12, WIND_ROW4 = WIND_ROW / 4, WIND_CHUNK = 1024;
constexpr float WIND_PI = 3.1415927410125732f, WIND_HALF_PI = 1.5707963705062866f;   // the fp32 neighbours of pi and pi / 2
constexpr float WIND_SCALE = 268435456.0f;                                            // 2^28: the fixed point of a term
// atan(r) = r * (c0 + c1 s + ... + c7 s^7), s = r * r, on [0, 1]; c0 is exactly 1 (include/dgs_mesh_ops.h says why)
constexpr float WIND_C0 = 1.0f, WIND_C1 = -0.3333165943622589f, WIND_C2 = 0.19962704181671143f, WIND_C3 = -0.13976581394672394f,
                WIND_C4 = 0.09794232249259949f, WIND_C5 = -0.05777356028556824f, WIND_C6 = 0.02304011397063732f,
                WIND_C7 = -0.004355399403721094f;

// atan2(y, x) of include/dgs_mesh_ops.h: 0 unless both are finite and one is not zero
__device__ __forceinline__ float wind_atan2(float y, float x) {
    const float ay = fabsf(y), ax = fabsf(x);
    const float mx = fmaxf(ay, ax), mn = fminf(ay, ax);
    const float r = mx > 0.0f ? mn / mx : 0.0f;                           // the IEEE division
    const float s = r * r;
    float p = WIND_C7;
    p = p * s + WIND_C6, p = p * s + WIND_C5, p = p * s + WIND_C4, p = p * s + WIND_C3;
    p = p * s + WIND_C2, p = p * s + WIND_C1, p = p * s + WIND_C0;
    p = p * r;
    p = ay > ax ? WIND_HALF_PI - p : p;
    p = x < 0.0f ? WIND_PI - p : p;
    p = y < 0.0f ? -p : p;
    const bool ok = (ay < __builtin_inff()) & (ax < __builtin_inff()) & (mx > 0.0f);   // false for a NaN
    return ok ? p : 0.0f;
}

__global__ __launch_bounds__(WIND_THREADS) void winding_sum_kernel(long long n_query, const float* __restrict__ query, long long n_tri,
                                                                   const float4* __restrict__ table, long long tri_chunk,
                                                                   unsigned long long* __restrict__ sums) {
    __shared__ float4 rows[WIND_T * WIND_ROW4];
    const long long q0 = (long long)blockIdx.x * WIND_Q + threadIdx.x;     // this thread's queries: q0 + k * WIND_THREADS
    const long long f_begin = (long long)blockIdx.y * tri_chunk;           // the host clamps tri_chunk to n_tri: no overflow
    const long long f_end = f_begin + tri_chunk < n_tri ? f_begin + tri_chunk : n_tri;
    float qx[WIND_K], qy[WIND_K], qz[WIND_K];
    long long acc[WIND_K];
#pragma unroll
    for (int k = 0; k < WIND_K; ++k) {
        const long long q = q0 + (long long)k * WIND_THREADS;
        const bool live = q < n_query;                                     // a thread past the end computes on zeros and stores nothing
        qx[k] = live ? query[3 * q] : 0.0f, qy[k] = live ? query[3 * q + 1] : 0.0f, qz[k] = live ? query[3 * q + 2] : 0.0f;
        acc[k] = 0;
    }
    for (long long fs = f_begin; fs < f_end; fs += WIND_T) {
        const int n = (int)(f_end - fs < WIND_T ? f_end - fs : WIND_T);   // rows of this round: only they are staged and read
        __syncthreads();                                                   // the previous round's readers are done
        const float4* src = table + fs * WIND_ROW4;
        for (int e = threadIdx.x; e < n * WIND_ROW4; e += WIND_THREADS)    // (fs + n) rows <= n_tri rows: inside the table;
            rows[e] = src[e];                                              // e < WIND_T * WIND_ROW4: inside the LDS array
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 r0 = rows[j * WIND_ROW4], r1 = rows[j * WIND_ROW4 + 1], r2 = rows[j * WIND_ROW4 + 2];
            // A = r0.xyz, B = (r0.w, r1.x, r1.y), C = (r1.z, r1.w, r2.x), n = r2.yzw
#pragma unroll
            for (int k = 0; k < WIND_K; ++k) {
                const float ax = r0.x - qx[k], ay = r0.y - qy[k], az = r0.z - qz[k];
                const float bx = r0.w - qx[k], by = r1.x - qy[k], bz = r1.y - qz[k];
                const float cx = r1.z - qx[k], cy = r1.w - qy[k], cz = r2.x - qz[k];
                const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)),
                            lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));      // (the IEEE sqrt)
                const float num = dot3(ax, ay, az, r2.y, r2.z, r2.w);
                const float ab = dot3(ax, ay, az, bx, by, bz), bc = dot3(bx, by, bz, cx, cy, cz), ca = dot3(cx, cy, cz, ax, ay, az);
                const float den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb);
                acc[k] += (long long)(int)rintf(wind_atan2(num, den) * WIND_SCALE);   // |theta| <= pi: the term is below 2^30
            }
        }
    }
#pragma unroll
    for (int k = 0; k < WIND_K; ++k) {
        const long long q = q0 + (long long)k * WIND_THREADS;
        if (q < n_query) atomicAdd(&sums[q], (unsigned long long)acc[k]);  // two's complement carries the sign
    }
}

// ---- earth mover's distance: the auction ------------------------------------------------------------------------------------------
// The fourth all-pairs search (dgs_emd_auction; include/dgs_mesh_ops.h states the quantity and the schedule, dgs_amd/mesh_metrics.py:
// emd_torch is the same statement in PyTorch).  Per unassigned person i, over ALL objects j: the smallest and the second smallest
// w = c_ij + p_j and the lowest j of the smallest -- a top-2 where nn_search_kernel keeps a top-1, with an integer price per point.
// Everything the auction iterates on is an integer: c_ij is an int in [0, 2^20], prices, bids and w are 64-bit.
//   packed word of an object = bid << 24 | bidder:  bidder < n < 2^24, bid < 2^39, the word below 2^63 like the packed minima above (a bid that would not fit raises the status flag
//   and is not placed).  The words are never cleared: a bid exceeds the price it is placed on (eps >= 1), the price is the last
//   winning bid, so every later word on an object is larger than every earlier one and an earlier one can never equal a new one.
// One round = two launches, the host enqueues them in batches (no kernel waits for another workgroup):
//   bid      every person of list[cur] finds its top-2 against the prices as they stand (nobody writes a price in this launch),
//            places atomicMax(word[j1], packed) and remembers (packed, j1);
//   resolve  every person of list[cur] looks at word[j1]: equal to its own packed word = it won (price, owner updated; the evicted
//            owner goes to list[cur ^ 1]), else it goes to list[cur ^ 1] itself.  Exactly one person wins an object, so owner[j] and
//            price[j] have one writer.  The order of a list depends on scheduling, nothing computed from it does.
// A round whose list is empty changes nothing (the bid launch only zeroes the other list's count, which is already 0), so rounds
// enqueued after a phase has converged are no-ops; `rounds` counts the launches that had bidders.
// Two bidding kernels, the same numbers (the host picks by the bidder count at the start of a batch; within a phase the count never
// grows: a round assigns as many persons as it evicts, or more):
//   dense   a thread per bidder (state in registers: coordinates, w1, j1, w2), the objects (x | y | z planes and the prices) staged
//           through LDS in rounds of EMD_T and read with 16-byte loads at an address every lane shares: a broadcast, as in
//           nn_search_kernel.  12 KB + 8 KB of LDS, 256 threads: occupancy is not the limit, the bidder count is -- the objects are
//           not sliced over workgroups (a packed minimum cannot carry a top-2, and the rounds that would need it are a handful).
//   sparse  a workgroup per bidder: thread t takes objects t, t + 256, ... straight from global memory (the whole set is n x 20
//           bytes, it lives in L2); a wave merges its 64 records by a butterfly of shuffles, the four waves meet in 96 bytes of LDS.
//           The walk is a chain of L2 round trips, so a round costs n / 256 of them (a wave per bidder, measured first, took 13 / 20 /
//           33 us per round at n = 2048 / 4096 / 8192: four times the trips).  EMD_SPARSE_MAX = 768 bidders are 768 workgroups = three
//           per CU, all resident at once.
// Per pair: 3 subtractions, 3 multiplications, 2 additions, a correctly rounded sqrt, multiply, rint, min, convert, a 64-bit add,
// two 64-bit compares and five selects.
constexpr int EMD_THREADS = 256, EMD_WAVES = EMD_THREADS / 64, EMD_T = 1024, EMD_SPARSE_MAX = 768;
constexpr int EMD_BIDDER_BITS = 24, EMD_BID_BITS = 39, EMD_MAX_BLOCKS = 1024;
constexpr float EMD_COST_CAP = 1048576.0f;                                   // 2^20
// the host's side (mesh_ops.hip): rounds per batch -- one read of the control block ends a batch; a phase leaves the dense rounds
// within a few of them, its sparse tail is hundreds to thousands long -- and the sizes of the caller's scratch and result arrays
constexpr int EMD_DENSE_BATCH = 4, EMD_SPARSE_BATCH = 64, EMD_RESULTS = 8, EMD_SCRATCH_FIXED = 64, EMD_SCRATCH_PER_POINT = 32;

struct EmdCtrl {                    // device-side control block, 64 bytes, zeroed by the host before the first launch
    int count[2];                   // persons in list[0], list[1]
    int status;                     // != 0: a bid did not fit EMD_BID_BITS
    int max_cost;                   // max c_ij (emd_max_cost_kernel)
    long long rounds;               // rounds that had bidders
    long long primal, sum_min, sum_price;   // emd_sums_kernel
    long long pad[2];
};
static_assert(sizeof(EmdCtrl) == EMD_SCRATCH_FIXED, "the control block is the fixed part of the scratch buffer");

struct EmdState {
    int n;
    float inv_q;
    const float *a, *b;             // [n,3] persons, objects
    long long* price;               // [n]
    unsigned long long *word, *mine;   // [n] per object: the largest packed bid so far;  [n] per person: its packed bid of this round (0: none)
    int *owner, *target, *assign;   // [n] object -> person or -1;  person -> the object it bid on;  person -> object (written at the end)
    int *list0, *list1;             // [n] each: the unassigned persons of this round and of the next (emd_list)
    EmdCtrl* ctrl;
};

struct EmdTop2 {
    long long w1, w2;               // smallest and second smallest c + p (over j != j1)
    int j1;                         // lowest index that attains w1
};

__device__ __forceinline__ int* emd_list(const EmdState& s, int k) { return k ? s.list1 : s.list0; }

__device__ __forceinline__ EmdTop2 emd_empty() { return EmdTop2{0x7FFFFFFFFFFFFFFFLL, 0x7FFFFFFFFFFFFFFFLL, 0x7FFFFFFF}; }

// c_ij = min(rint(sqrt((dx dx + dy dy) + dz dz) * inv_q), 2^20): every operation rounded on its own, the sqrt correctly rounded
__device__ __forceinline__ int emd_cost(float ax, float ay, float az, float bx, float by, float bz, float inv_q) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);              // (the IEEE sqrt; __fsqrt_rn is v_sqrt_f32 here: 1 ulp)
    return (int)fminf(rintf(d * inv_q), EMD_COST_CAP);
}

// objects are visited in ascending j: the strict `<` keeps the lowest index among equal w1
__device__ __forceinline__ void emd_visit(EmdTop2& t, long long w, int j) {
    const bool first = w < t.w1, second = w < t.w2;
    t.w2 = first ? t.w1 : (second ? w : t.w2);
    t.j1 = first ? j : t.j1;
    t.w1 = first ? w : t.w1;
}

// the top-2 of the union of two disjoint object sets; symmetric in its arguments
__device__ __forceinline__ EmdTop2 emd_merge(const EmdTop2& x, const EmdTop2& y) {
    const bool swap = y.w1 < x.w1 || (y.w1 == x.w1 && y.j1 < x.j1);
    EmdTop2 lo = swap ? y : x;
    const long long other = swap ? x.w1 : y.w1;
    lo.w2 = lo.w2 < other ? lo.w2 : other;
    return lo;
}

__device__ __forceinline__ EmdTop2 emd_wave_merge(EmdTop2 t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        EmdTop2 o;
        o.w1 = __shfl_xor(t.w1, m, 64), o.w2 = __shfl_xor(t.w2, m, 64), o.j1 = __shfl_xor(t.j1, m, 64);
        t = emd_merge(t, o);
    }
    return t;                                                              // the same record in every lane
}

// one thread's walk over objects first, first + stride, ... (inside [0, n)) for the person at (ax, ay, az), merged over its wave.
// Four objects are loaded before the first is used: the loads of a step overlap instead of queueing behind each other's use.
__device__ __forceinline__ EmdTop2 emd_wave_scan(const EmdState& s, float ax, float ay, float az, int first, int stride) {
    EmdTop2 t = emd_empty();
    int j = first;
    for (; j + 3 * stride < s.n; j += 4 * stride) {
        float x[4], y[4], z[4];
        long long p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j + u * stride;                                  // <= j + 3 stride < n
            x[u] = s.b[3 * k], y[u] = s.b[3 * k + 1], z[u] = s.b[3 * k + 2], p[u] = s.price[k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) emd_visit(t, (long long)emd_cost(ax, ay, az, x[u], y[u], z[u], s.inv_q) + p[u], j + u * stride);
    }
    for (; j < s.n; j += stride)
        emd_visit(t, (long long)emd_cost(ax, ay, az, s.b[3 * j], s.b[3 * j + 1], s.b[3 * j + 2], s.inv_q) + s.price[j], j);
    return emd_wave_merge(t);
}

// the four waves of a workgroup meet in LDS; the result in every thread.  `slot`: EMD_WAVES records of the caller's LDS.
__device__ __forceinline__ EmdTop2 emd_group_merge(EmdTop2 t, EmdTop2* slot) {
    __syncthreads();                                                       // the readers of an earlier use are done
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = t;
    __syncthreads();
    EmdTop2 r = slot[0];
#pragma unroll
    for (int w = 1; w < EMD_WAVES; ++w) r = emd_merge(r, slot[w]);
    return r;
}

// n >= 2: j1 is an object and w2 a real value.  bid = p_j1 + (w2 - w1) + eps >= 1.
__device__ __forceinline__ void emd_place(const EmdState& s, int i, const EmdTop2& t, long long eps) {
    const long long bid = s.price[t.j1] + (t.w2 - t.w1) + eps;
    unsigned long long packed = 0;
    if (bid < (1LL << EMD_BID_BITS)) {
        packed = ((unsigned long long)bid << EMD_BIDDER_BITS) | (unsigned long long)i;
        atomicMax(&s.word[t.j1], packed);
    } else {
        atomicOr(&s.ctrl->status, 1);
    }
    s.mine[i] = packed, s.target[i] = t.j1;
}

__global__ __launch_bounds__(EMD_THREADS) void emd_bid_dense_kernel(EmdState s, int cur, long long eps) {
    __shared__ __attribute__((aligned(16))) float pts[3 * EMD_T];
    __shared__ __attribute__((aligned(16))) long long prc[EMD_T];
    const int count = s.ctrl->count[cur];                                  // <= n; nobody writes it during this launch
    if (blockIdx.x == 0 && threadIdx.x == 0) s.ctrl->count[cur ^ 1] = 0;   // the list the resolve launch will fill
    for (int first = blockIdx.x * EMD_THREADS; first < count; first += gridDim.x * EMD_THREADS) {   // (uniform over the workgroup)
        const int t = first + threadIdx.x;
        const bool live = t < count;                                       // a thread past the end computes on person 0 and places nothing
        const int i = live ? emd_list(s, cur)[t] : 0;
        const float ax = s.a[3 * i], ay = s.a[3 * i + 1], az = s.a[3 * i + 2];
        EmdTop2 r = emd_empty();
        auto visit = [&](float x, float y, float z, long long p, int j) { emd_visit(r, (long long)emd_cost(ax, ay, az, x, y, z, s.inv_q) + p, j); };
        for (int js = 0; js < s.n; js += EMD_T) {
            const int m = s.n - js < EMD_T ? s.n - js : EMD_T;            // objects of this round: only they are staged and read
            __syncthreads();                                               // the previous round's readers are done
            const float* src = s.b + 3 * js;
            for (int e = threadIdx.x; e < 3 * m; e += EMD_THREADS) {       // 3 (js + m) <= 3 n: inside the object array
                const int p = e / 3;
                pts[(e - 3 * p) * EMD_T + p] = src[e];
            }
            for (int e = threadIdx.x; e < m; e += EMD_THREADS) prc[e] = s.price[js + e];
            __syncthreads();
            int j = 0;
            for (; j + 4 <= m; j += 4) {
                const float4 X = *reinterpret_cast<const float4*>(&pts[j]), Y = *reinterpret_cast<const float4*>(&pts[EMD_T + j]),
                             Z = *reinterpret_cast<const float4*>(&pts[2 * EMD_T + j]);
                visit(X.x, Y.x, Z.x, prc[j], js + j), visit(X.y, Y.y, Z.y, prc[j + 1], js + j + 1);
                visit(X.z, Y.z, Z.z, prc[j + 2], js + j + 2), visit(X.w, Y.w, Z.w, prc[j + 3], js + j + 3);
            }
            for (; j < m; ++j) visit(pts[j], pts[EMD_T + j], pts[2 * EMD_T + j], prc[j], js + j);
        }
        if (live) emd_place(s, i, r, eps);
    }
}

__global__ __launch_bounds__(EMD_THREADS) void emd_bid_sparse_kernel(EmdState s, int cur, long long eps) {
    const int count = s.ctrl->count[cur];
    if (blockIdx.x == 0 && threadIdx.x == 0) s.ctrl->count[cur ^ 1] = 0;
    __shared__ EmdTop2 slot[EMD_WAVES];
    for (int t = blockIdx.x; t < count; t += gridDim.x) {                  // (uniform over the workgroup: the barriers are met by all)
        const int i = emd_list(s, cur)[t];
        const EmdTop2 r = emd_group_merge(emd_wave_scan(s, s.a[3 * i], s.a[3 * i + 1], s.a[3 * i + 2], threadIdx.x, EMD_THREADS), slot);
        if (threadIdx.x == 0) emd_place(s, i, r, eps);
    }
}

__global__ __launch_bounds__(EMD_THREADS) void emd_resolve_kernel(EmdState s, int cur) {
    const int count = s.ctrl->count[cur];
    if (blockIdx.x == 0 && threadIdx.x == 0 && count > 0) s.ctrl->rounds += 1;   // (its only writer; read by the host)
    for (int t = blockIdx.x * EMD_THREADS + threadIdx.x; t < count; t += gridDim.x * EMD_THREADS) {
        const int i = emd_list(s, cur)[t], j = s.target[i];
        const unsigned long long packed = s.mine[i];
        int back = i;                                                      // who is unassigned after this round: the loser itself ...
        if (packed != 0 && s.word[j] == packed) {
            s.price[j] = (long long)(packed >> EMD_BIDDER_BITS);
            back = s.owner[j];                                             // ... or the owner the winner evicts (-1: the object was free)
            s.owner[j] = i;
        }
        if (back >= 0) emd_list(s, cur ^ 1)[atomicAdd(&s.ctrl->count[cur ^ 1], 1)] = back;   // at most `count` <= n appends
    }
}

// the start of a phase: nobody assigned, the prices stay
__global__ __launch_bounds__(EMD_THREADS) void emd_phase_kernel(EmdState s) {
    const int i = blockIdx.x * EMD_THREADS + threadIdx.x;
    if (i < s.n) s.owner[i] = -1, s.list0[i] = i;
    if (i == 0) s.ctrl->count[0] = s.n, s.ctrl->count[1] = 0;
}

// max c_ij, for the first eps: a wave per person, one atomic per wave
__global__ __launch_bounds__(EMD_THREADS) void emd_max_cost_kernel(EmdState s) {
    const int lane = threadIdx.x & 63;
    int best = 0;
    for (int i = blockIdx.x * EMD_WAVES + (threadIdx.x >> 6); i < s.n; i += gridDim.x * EMD_WAVES) {
        const float ax = s.a[3 * i], ay = s.a[3 * i + 1], az = s.a[3 * i + 2];
        for (int j = lane; j < s.n; j += 64) {
            const int c = emd_cost(ax, ay, az, s.b[3 * j], s.b[3 * j + 1], s.b[3 * j + 2], s.inv_q);
            best = c > best ? c : best;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(best, m, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) atomicMax(&s.ctrl->max_cost, best);
}

__global__ __launch_bounds__(EMD_THREADS) void emd_assign_kernel(EmdState s) {
    const int j = blockIdx.x * EMD_THREADS + threadIdx.x;
    if (j < s.n) {
        const int i = s.owner[j];
        if (i >= 0 && i < s.n) s.assign[i] = j;                            // (a permutation when the auction has ended)
    }
}

// primal = sum_i c_{i, assign(i)};  sum_min = sum_i min_j (c_ij + p_j), the bidding pass's first half;  sum_price = sum_j p_j.
// Integer sums: a wave adds up its persons in registers and issues three 64-bit atomic adds; any order gives the same integers.
__global__ __launch_bounds__(EMD_THREADS) void emd_sums_kernel(EmdState s) {
    const int lane = threadIdx.x & 63;
    long long primal = 0, sum_min = 0, sum_price = 0;
    for (int i = blockIdx.x * EMD_WAVES + (threadIdx.x >> 6); i < s.n; i += gridDim.x * EMD_WAVES) {
        const float ax = s.a[3 * i], ay = s.a[3 * i + 1], az = s.a[3 * i + 2];
        const EmdTop2 r = emd_wave_scan(s, ax, ay, az, lane, 64);
        const int j0 = s.assign[i];                                        // -1 (the host's fill) if the owners were no permutation:
        const int j = (unsigned)j0 < (unsigned)s.n ? j0 : 0;               // flagged, and no address leaves the object array
        if (j != j0 && lane == 0) atomicOr(&s.ctrl->status, 2);
        sum_min += r.w1, sum_price += s.price[i];
        primal += emd_cost(ax, ay, az, s.b[3 * j], s.b[3 * j + 1], s.b[3 * j + 2], s.inv_q);
    }
    if (lane == 0) {
        atomicAdd((unsigned long long*)&s.ctrl->primal, (unsigned long long)primal);
        atomicAdd((unsigned long long*)&s.ctrl->sum_min, (unsigned long long)sum_min);
        atomicAdd((unsigned long long*)&s.ctrl->sum_price, (unsigned long long)sum_price);
    }
}

}  // namespace
