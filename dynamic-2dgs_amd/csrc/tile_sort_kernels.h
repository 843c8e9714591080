// tile_sort_kernels.h -- the per-tile sorts of the bucketed keys into point_list (gfx950): bitonic network in LDS and in registers,
// LSD radix sort in LDS (the default), segment merge for lists above one workgroup's capacity, global-memory fallback.
// Replaces cub DeviceRadixSort of the reference (rasterizer_impl.cu:304-319); the order is the same (binning_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dgs {

// Per-tile sort by (depth, index): one workgroup per tile, bitonic network on 64-bit keys.
//   sort_tiles_lds_kernel<CAP>: buckets with lo < n <= CAP are padded to a power of two and sorted in LDS
//       (CAP = 2048 -> 16 KB and ten resident workgroups per CU, the common case: a few hundred entries;
//        CAP = 16384 -> 128 KB for crowded tiles);
//   sort_tiles_global_kernel: buckets longer than that are copied, padded, into scratch [2*start, 2*start + n2)
//       (disjoint across tiles because n2 < 2n) and sorted there by the same network -- slow, but only reachable
//       by degenerate views (tens of thousands of surfels over one tile).
// Thread i of a pass handles the pair (l, l + j) with l = ((i & ~(j-1)) << 1) | (i & (j-1)).  For j <= 64 the 64 pairs
// of a wave (i = 64w .. 64w+63, and again every 256) live in the wave's own 128-key window, so consecutive stages with
// j <= 64 need no workgroup barrier -- only the LDS ordering of a single wave.  A 1024-key sort keeps 9 of its 55 barriers.  (`wave_local` must be false when `k` is global memory.)
__device__ __forceinline__ void bitonic_network(uint64_t* k, int n2, int tid, bool wave_local)
{
    const int half = n2 >> 1;
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            // four independent pairs per thread and trip: all eight loads are in flight before the first compare
            for (int i0 = tid; i0 < half; i0 += 1024) {
                int l[4];
                uint64_t a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + 256 * u;
                    l[u] = ((i & ~(j - 1)) << 1) | (i & (j - 1));  // j is a power of two
                    if (i < half) { a[u] = k[l[u]]; b[u] = k[l[u] + j]; }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + 256 * u;
                    const bool up = (l[u] & kk) == 0;
                    if (i < half && (a[u] > b[u]) == up) { k[l[u]] = b[u]; k[l[u] + j] = a[u]; }
                }
            }
            // the next stage is (kk, j/2), or (2kk, kk) after j == 1; a workgroup barrier is needed only when this
            // stage or the next one crosses the 128-key windows (stride > 64)
            const int j_next = j > 1 ? (j >> 1) : kk;
            if (wave_local && j <= 64 && j_next <= 64) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            else __syncthreads();
        }
}

template <int CAP>
__global__ void __launch_bounds__(256) sort_tiles_lds_kernel(const uint2* ranges, const uint64_t* keys, uint32_t* point_list, int lo)
{
    __shared__ uint64_t s_keys[CAP];
    const uint2 rg = ranges[blockIdx.x];
    const int n = (int)(rg.y - rg.x);
    if (n <= lo || n > CAP) return;
    const uint64_t* gk = keys + rg.x;
    const int tid = threadIdx.x;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n2; i += 256) s_keys[i] = i < n ? gk[i] : ~0ull;
    __syncthreads();
    bitonic_network(s_keys, n2, tid, true);
    for (int i = tid; i < n; i += 256) point_list[rg.x + i] = (uint32_t)s_keys[i];
}

// Register-resident variant for buckets of up to 2048 entries (the common case; the LDS network above spends its time in
// the LDS pipe: four 64-bit LDS operations per compared pair and stage).  Thread t of the 256 keeps the keys of elements
// t + 256 s (s < SLOTS) in registers; the partner of element e in stage (kk, j) is e ^ j, and e keeps the smaller key iff
// ((e & j) == 0) == ((e & kk) == 0).  So
//   j >= 256 : the partner is another slot of the same thread  -> compare-exchange in registers, no data movement;
//   j <  64  : the partner is the same slot of lane ^ j        -> two ds_bpermute per key;
//   j = 64, 128 : another wave                                 -> one round trip through LDS (9 of the 66 stages at 2048).
// Value of `v` in lane (lane ^ j): two ds_bpermute.  (DPP quad permutes / bank-masked row shifts for j <= 8 were measured and
// are slower: 76 us against 49 us for the kernel at 200 k surfels -- the VALU, not the LDS pipe, is what the network saturates.)
__device__ __forceinline__ uint64_t lane_xor_u64(uint64_t v, int j)
{
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    return ((uint64_t)(uint32_t)__shfl_xor((int)hi, j, 64) << 32) | (uint32_t)__shfl_xor((int)lo, j, 64);
}

template <int SLOTS, int DS>
__device__ __forceinline__ void sort_cx_slots(uint64_t (&k)[SLOTS], int kk, int tid)
{
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        if (s & DS) continue;
        const bool up = ((tid + 256 * s) & kk) == 0;
        const uint64_t a = k[s], b = k[s | DS];
        const bool sw = (a > b) == up;
        k[s] = sw ? b : a;
        k[s | DS] = sw ? a : b;
    }
}

template <int SLOTS>
__device__ __forceinline__ void sort_tile_regs(uint64_t* s_keys, const uint64_t* gk, int n, uint32_t* out, int tid)
{
    uint64_t k[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = tid + 256 * s;
        k[s] = e < n ? gk[e] : ~0ull;
    }
    for (int kk = 2; kk <= 256 * SLOTS; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j >= 256) {
                if constexpr (SLOTS >= 2) { if (j == 256) sort_cx_slots<SLOTS, 1>(k, kk, tid); }
                if constexpr (SLOTS >= 4) { if (j == 512) sort_cx_slots<SLOTS, 2>(k, kk, tid); }
                if constexpr (SLOTS >= 8) { if (j == 1024) sort_cx_slots<SLOTS, 4>(k, kk, tid); }
                continue;
            }
            const bool lower = (tid & j) == 0;
            if (j >= 64) {
#pragma unroll
                for (int s = 0; s < SLOTS; s++) s_keys[tid + 256 * s] = k[s];
                __syncthreads();
#pragma unroll
                for (int s = 0; s < SLOTS; s++) {
                    const uint64_t p = s_keys[(tid ^ j) + 256 * s];
                    const bool keep_min = lower == ((((tid + 256 * s) & kk)) == 0);
                    k[s] = ((p < k[s]) == keep_min) ? p : k[s];
                }
                __syncthreads();
            } else {
#pragma unroll
                for (int s = 0; s < SLOTS; s++) {
                    const uint64_t p = lane_xor_u64(k[s], j);
                    const bool keep_min = lower == ((((tid + 256 * s) & kk)) == 0);
                    k[s] = ((p < k[s]) == keep_min) ? p : k[s];
                }
            }
        }
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
        const int e = tid + 256 * s;
        if (e < n) out[e] = (uint32_t)k[s];
    }
}

__global__ void __launch_bounds__(256) sort_tiles_reg_kernel(const uint2* ranges, const uint64_t* keys, uint32_t* point_list)
{
    __shared__ uint64_t s_keys[2048];
    const uint2 rg = ranges[blockIdx.x];
    const int n = (int)(rg.y - rg.x);
    if (n <= 0 || n > 2048) return;
    const uint64_t* gk = keys + rg.x;
    uint32_t* out = point_list + rg.x;
    const int tid = threadIdx.x;
    if (n <= 256) sort_tile_regs<1>(s_keys, gk, n, out, tid);
    else if (n <= 512) sort_tile_regs<2>(s_keys, gk, n, out, tid);
    else if (n <= 1024) sort_tile_regs<4>(s_keys, gk, n, out, tid);
    else sort_tile_regs<8>(s_keys, gk, n, out, tid);
}

// ---- per-tile radix sort ---------------------------------------------------------------------------------------------
// One workgroup per tile bucket, LSD radix on the depth bits with 8-bit digits, everything in LDS:
//   * only the bits that DIFFER inside the bucket are sorted: depths of one tile share sign, most of the exponent and often
//     more (xor of the bucket's min and max), typically 3 passes instead of 4;
//   * a pass is a stable counting sort: wave w owns a contiguous quarter of the bucket; for each of its 64-element slots the
//     lanes that hold the same digit find each other with 8 ballots (one per digit bit), rank = population count of the
//     peers below the lane, a wave-private LDS histogram carries the running count from slot to slot; the 4 x 256 wave
//     histograms are scanned by the 256 threads (digit-major, then wave) and every element is written to its final place;
//   * the (depth, surfel index) order of the reference's stable radix sort (rasterizer_impl.cu:304-309: ties in depth keep the
//     emission order = ascending surfel index) is restored at the end: the bucket arrives in arbitrary order, so equal
//     depths -- exact float equality, i.e. duplicated surfels -- come out in arbitrary order; each such run is sorted by
//     index by the thread that finds its head.
// O(n) operations per pass instead of the O(n log^2 n) compare-exchanges of the bitonic network (which saturated the VALU:
// 62 us at 200 k surfels / 800x800); keys are 32-bit here (depth bits; the index rides along as payload).
// SEG = true (lists longer than CAP): blockIdx.y = segment; the workgroup sorts entries [y CAP, (y + 1) CAP) of every list of
// more than CAP and at most CAP * gridDim.y entries and writes the sorted (depth, index) KEYS into the list's scratch area;
// merge_segments_kernel then ranks every key among the other segments.  `seg_out` = scratch of 2 R keys (list at 2 * range.x).
// CAP = kSegCap = 2048 (36 KB of LDS), up to kMaxSegs = 28 segments per list.  History: round 3 used segments of 3584 (60 KB); the
// 8192-entry / 132-KB instantiation that round 2 used for lists of 2 k - 8 k entries never took less than ~73 us per launch, with or
// without work (36 workgroups that find nothing to sort: 73 us; the segment kernel: 2 us).  The cause was not isolated -- bare
// allocations of 16 .. 160 KB launch in 2.5 us whatever their size (tools/micro/lds_launch_bench.hip) -- the smaller instantiations do
// not show it, and their segments run side by side.
// Round 4: the segments are as long as the main kernel's lists (2048) and EVERY list beyond that is cut into them -- the 3584-entry
// single-workgroup instantiation that used to take the lists of 2 049 .. 3 584 entries is gone: one workgroup of four waves needs
// 25-50 us for such a list (the launch a densified scene waited for), two or more segments side by side + the rank / merge step half.
constexpr int kSegCap = 2048;
constexpr int kMaxSegs = 28;
template <int CAP, bool SEG = false>
__global__ void __launch_bounds__(256) sort_tiles_radix_kernel(const uint2* ranges, int ntiles, const uint64_t* keys, uint32_t* point_list, int lo,
                                                               uint64_t* seg_out = nullptr, const uint32_t* state = nullptr /*[1] = longest list*/)
{
    if (SEG && state && (uint32_t)blockIdx.y * (uint32_t)CAP >= state[1]) return;   // no list of this launch reaches this segment index
    __shared__ uint32_t s_key[2][CAP];
    __shared__ uint32_t s_val[2][CAP];
    __shared__ uint32_t s_hist[4][256];      // per wave: running digit counts, then exclusive global offsets
    __shared__ uint32_t s_red[8];
    // grid-stride over the tiles: the launch for long lists uses a small grid (a 132 KB workgroup per tile that exits at once
    // would cost ten dispatch rounds of 2500 workgroups for nothing)
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint2 rg = ranges[tile];
    const int n_list = (int)(rg.y - rg.x);
    const int seg0 = SEG ? (int)blockIdx.y * CAP : 0;
    if (SEG ? (n_list <= CAP || n_list > CAP * (int)gridDim.y || seg0 >= n_list) : (n_list <= lo || n_list > CAP)) continue;
    const int n = SEG ? min(CAP, n_list - seg0) : n_list;
    __syncthreads();   // the previous tile's last reads of the LDS arrays
    const uint64_t* gk = keys + rg.x + seg0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- load, and the bits in which the bucket's depths differ
    uint32_t kand = 0xffffffffu, kor = 0u;
    {
        // all of the thread's keys are requested before the first is used (a load -> LDS store loop is one memory round trip per
        // trip: three for the average list of the metric scene, of a kernel whose workgroups run in 2.4 rounds)
        constexpr int kLoads = CAP / 256;
        uint64_t kb[kLoads];
#pragma unroll
        for (int l = 0; l < kLoads; l++) { const int i = tid + 256 * l; kb[l] = i < n ? gk[i] : 0ull; }
#pragma unroll
        for (int l = 0; l < kLoads; l++) {
            const int i = tid + 256 * l;
            if (i < n) {
                const uint32_t d = (uint32_t)(kb[l] >> 32);
                s_key[0][i] = d;
                s_val[0][i] = (uint32_t)kb[l];
                kand &= d; kor |= d;
            }
        }
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) {
        kand &= (uint32_t)__shfl_xor((int)kand, sft, 64);
        kor |= (uint32_t)__shfl_xor((int)kor, sft, 64);
    }
    if (lane == 0) { s_red[wave] = kand; s_red[4 + wave] = kor; }
    __syncthreads();
    const uint32_t diff = (s_red[0] & s_red[1] & s_red[2] & s_red[3]) ^ (s_red[4] | s_red[5] | s_red[6] | s_red[7]);
    const int nbits = diff ? 32 - __builtin_clz(diff) : 0;
    // wave w owns elements [w0, w1): contiguous, so array order == (wave, slot, lane) order
    const int per = (n + 3) >> 2;
    const int w0 = wave * per, w1 = min(n, w0 + per);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int cur = 0;
    for (int shift = 0; shift < nbits; shift += 8, cur ^= 1) {
        s_hist[wave][lane] = 0; s_hist[wave][lane + 64] = 0; s_hist[wave][lane + 128] = 0; s_hist[wave][lane + 192] = 0;
        // (wave-private rows: the wave's own LDS operations are ordered, no barrier needed before the first slot)
        const uint32_t* kin = s_key[cur];
        const uint32_t* vin = s_val[cur];
        // ---- rank inside the wave's range
        constexpr int kMaxSlots = (CAP / 4 + 63) / 64;
        uint32_t my_rank[kMaxSlots];      // rank of my element of slot e among the wave's elements with the same digit
#pragma unroll
        for (int e = 0; e < kMaxSlots; e++) {
            const int pos = w0 + e * 64 + lane;
            if (w0 + e * 64 >= w1) break;                     // wave-uniform
            const bool live = pos < w1;
            const uint32_t d = live ? ((kin[pos] >> shift) & 255u) : 256u;   // 256: no peer among the live lanes
            unsigned long long peers = __ballot(live);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const unsigned long long bal = __ballot((d >> b) & 1u);
                peers &= ((d >> b) & 1u) ? bal : ~bal;
            }
            const uint32_t below = (uint32_t)__popcll(peers & lt_mask), total = (uint32_t)__popcll(peers);
            uint32_t base = 0;
            if (live) base = s_hist[wave][d];
            my_rank[e] = base + below;
            if (live && below == 0) s_hist[wave][d] = base + total;   // one leader per digit
        }
        __syncthreads();
        // ---- exclusive offsets over (digit, wave): thread t = digit t
        {
            const uint32_t c0 = s_hist[0][tid], c1 = s_hist[1][tid], c2 = s_hist[2][tid], c3 = s_hist[3][tid];
            const uint32_t tot = c0 + c1 + c2 + c3;
            uint32_t inc = tot;
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)inc, dd, 64);
                if (lane >= dd) inc += up;
            }
            if (lane == 63) s_red[wave] = inc;
            __syncthreads();
            uint32_t off = inc - tot;
            for (int w = 0; w < wave; w++) off += s_red[w];
            s_hist[0][tid] = off; s_hist[1][tid] = off + c0; s_hist[2][tid] = off + c0 + c1; s_hist[3][tid] = off + c0 + c1 + c2;
        }
        __syncthreads();
        // ---- scatter
        uint32_t* kout = s_key[cur ^ 1];
        uint32_t* vout = s_val[cur ^ 1];
#pragma unroll
        for (int e = 0; e < kMaxSlots; e++) {
            const int pos = w0 + e * 64 + lane;
            if (w0 + e * 64 >= w1) break;
            if (pos < w1) {
                const uint32_t k = kin[pos];
                const uint32_t dst = s_hist[wave][(k >> shift) & 255u] + my_rank[e];
                kout[dst] = k;
                vout[dst] = vin[pos];
            }
        }
        __syncthreads();
    }
    // ---- ties in depth: ascending surfel index (the head of a run sorts it; runs are duplicated surfels, i.e. short)
    uint32_t* kf = s_key[cur];
    uint32_t* vf = s_val[cur];
    for (int i = tid; i < n - 1; i += 256) {
        if (kf[i] == kf[i + 1] && (i == 0 || kf[i - 1] != kf[i])) {
            int end = i + 2;
            while (end < n && kf[end] == kf[i]) end++;
            for (int a = i + 1; a < end; a++) {          // insertion sort of vf[i, end)
                const uint32_t v = vf[a];
                int b = a - 1;
                while (b >= i && vf[b] > v) { vf[b + 1] = vf[b]; b--; }
                vf[b + 1] = v;
            }
        }
    }
    __syncthreads();
    if (SEG) {
        uint64_t* so = seg_out + 2 * (size_t)rg.x + seg0;
        for (int i = tid; i < n; i += 256) so[i] = ((uint64_t)kf[i] << 32) | vf[i];
    } else {
        for (int i = tid; i < n; i += 256) point_list[rg.x + i] = vf[i];
    }
    }
}

// Lists of more than kSegCap entries, second step: every key of segment y finds its place in the whole list -- its index in
// its own (sorted) segment plus, for every other segment, the number of keys below it.  Keys are unique inside a list (the
// surfel index is part of the key), so "below" needs no tie rule and the result is the reference's stable (depth, index) order.
// A thread owns 8 CONSECUTIVE keys of its segment; the other segments pass through LDS one at a time (17 KB, coalesced load):
// the number of its keys below each of the thread's keys is a branch-free binary search in LDS.
// Searching the other segments where they lie, in global memory, is a chain of ~200 dependent loads per thread: 0.67 ms.
// (LDS index i lives at i + i / 32: the threads' search positions are ~32 keys apart, which would be one bank.)
__global__ void __launch_bounds__(256) merge_segments_kernel(const uint2* ranges, int ntiles, const uint64_t* seg_keys /*scratch*/, uint32_t* point_list,
                                                             const uint32_t* state /*[1] = longest list*/)
{
    if ((uint32_t)blockIdx.y * (uint32_t)kSegCap >= state[1]) return;   // no list of this launch reaches this segment index
    constexpr int kPer = kSegCap / 256;
    __shared__ uint64_t s_other[kSegCap + kSegCap / 32];
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint2 rg = ranges[tile];
        const int n_list = (int)(rg.y - rg.x);
        const int seg = (int)blockIdx.y, seg0 = seg * kSegCap;
        if (n_list <= kSegCap || n_list > kSegCap * (int)gridDim.y || seg0 >= n_list) continue;   // (workgroup-uniform)
        const uint64_t* base = seg_keys + 2 * (size_t)rg.x;
        const int n = min(kSegCap, n_list - seg0), nseg = (n_list + kSegCap - 1) / kSegCap;
        const int i0 = (int)threadIdx.x * kPer, cnt = max(0, min(kPer, n - i0));
        uint64_t mine[kPer];
        int rank[kPer];
#pragma unroll
        for (int i = 0; i < kPer; i++) { mine[i] = i < cnt ? base[seg0 + i0 + i] : ~0ull; rank[i] = i0 + i; }
        for (int o = 0; o < nseg; o++) {
            if (o == seg) continue;
            const int len = min(kSegCap, n_list - o * kSegCap);
            __syncthreads();
            for (int i = threadIdx.x; i < len; i += 256) s_other[i + (i >> 5)] = base[o * kSegCap + i];
            __syncthreads();
            // branch-free lower bound of all 8 keys at once: 12 rounds of 8 independent LDS reads (a merge-style walk from key to
            // key is a chain of dependent reads inside a divergent loop: 25 us per segment instead of ~2)
            int pos[kPer];
#pragma unroll
            for (int i = 0; i < kPer; i++) pos[i] = 0;
#pragma unroll
            for (int step = 2048; step >= 1; step >>= 1) {
#pragma unroll
                for (int i = 0; i < kPer; i++) {
                    const int p = pos[i] + step;
                    const int q = p <= len ? p - 1 : 0;
                    const bool below = (p <= len) & (s_other[q + (q >> 5)] < mine[i]);
                    pos[i] = below ? p : pos[i];
                }
            }
#pragma unroll
            for (int i = 0; i < kPer; i++) rank[i] += pos[i];   // (padding keys of a thread with fewer than 8 are never written)
        }
#pragma unroll
        for (int i = 0; i < kPer; i++)
            if (i < cnt) point_list[rg.x + rank[i]] = (uint32_t)mine[i];
    }
}

__global__ void __launch_bounds__(256) sort_tiles_global_kernel(const uint2* ranges, int ntiles, const uint64_t* keys, uint64_t* scratch /*[2R]*/,
                                                                uint32_t* point_list, int lo)
{
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // grid-stride: launched with a small grid
        const uint2 rg = ranges[tile];
        const int n = (int)(rg.y - rg.x);
        if (n <= lo) continue;
        const uint64_t* gk = keys + rg.x;
        uint64_t* sk = scratch + 2 * (size_t)rg.x;
        const int tid = threadIdx.x;
        int n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (int i = tid; i < n2; i += 256) sk[i] = i < n ? gk[i] : ~0ull;
        __syncthreads();
        bitonic_network(sk, n2, tid, false);
        for (int i = tid; i < n; i += 256) point_list[rg.x + i] = (uint32_t)sk[i];
        __syncthreads();
    }
}

}  // namespace dgs
