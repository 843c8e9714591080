// tile_order_kernels.h -- the dispatch order of the blend kernels' tiles (tile orders 3 and 4 of blend_common.h tile_for_block):
// counting sorts of the tiles by list length (forward) or traversed length (backward), as bodies that the binning kernels call
// from their last workgroup (binning_kernels.h), as a kernel of their own, and fused with the backward's accumulator clear.
#pragma once
#include <hip/hip_runtime.h>

namespace dgs {

// Mode 3 (default): longest-processing-time-first.  Tile work varies by >10x (empty corners vs the dense centre)
// and a workgroup owns its tile to the end, so with ~7 resident workgroups per CU the kernel time is set by
// whichever SIMD drew the heaviest tiles last.  Dispatching tiles in descending list length (counting sort below)
// puts the long tiles first and lets the short ones fill the tail.
constexpr int kOrderBins = 1024;
constexpr int kOrderGroup = 4;      // mode 4: tiles per group edge
constexpr int kOrderMaxGroups = 1024;
// mode 4: slots of the order array = 8 x (most tiles one XCD can get): every XCD gets at most ceil(G / 8) + 1 groups of 16 tiles
__host__ __device__ inline int order_groups(int tiles_x, int tiles_y)
{
    return ((tiles_x + kOrderGroup - 1) / kOrderGroup) * ((tiles_y + kOrderGroup - 1) / kOrderGroup);
}
__host__ __device__ inline int order_slots(int tiles_x, int tiles_y)
{
    return 8 * kOrderGroup * kOrderGroup * ((order_groups(tiles_x, tiles_y) + 7) / 8 + 1);
}

// body shared by tile_order_kernel and scan_tiles_kernel (which orders the forward's tiles right after it has scanned their
// counts: one launch less in the step); all 1024 threads of the workgroup must call it
__device__ __forceinline__ void tile_order_body(const uint2* ranges, const uint32_t* weights, int ntiles, uint32_t* order, uint32_t* s_hist /*[kOrderBins]*/,
                                                uint32_t* s_wsum /*[16]*/)
{
    const int tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    // bin 0 = heaviest.  weight = list length (ranges) or traversed length (weights), 4 entries per bin, saturating.
    // Both passes take four tiles per thread and trip with all four loads in flight (this body is the serial tail of the launch it
    // rides in -- one workgroup, the rest of the device idle: a load -> LDS atomic loop was one memory round trip per 1024 tiles
    // and pass, five at 2500 tiles)
    auto weight4 = [&](int t0, uint32_t (&w)[4]) {
#pragma unroll
        for (int l = 0; l < 4; l++) {
            const int t = t0 + 1024 * l;
            if (weights) w[l] = t < ntiles ? weights[t] : 0u;
            else { const uint2 r = t < ntiles ? ranges[t] : make_uint2(0u, 0u); w[l] = r.y - r.x; }
        }
    };
    for (int t0 = tid; t0 < ntiles; t0 += 4096) {
        uint32_t w[4];
        weight4(t0, w);
#pragma unroll
        for (int l = 0; l < 4; l++)
            if (t0 + 1024 * l < ntiles) atomicAdd(&s_hist[kOrderBins - 1 - min(w[l] >> 2, (uint32_t)(kOrderBins - 1))], 1u);
    }
    __syncthreads();
    // exclusive scan of the 1024 bins (one per thread)
    const uint32_t v = s_hist[tid];
    uint32_t inc = v;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t n = __shfl_up(inc, d, 64);
        if (lane >= d) inc += n;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += s_wsum[w];
    __syncthreads();
    s_hist[tid] = base + inc - v;
    __syncthreads();
    for (int t0 = tid; t0 < ntiles; t0 += 4096) {
        uint32_t w[4], pos[4];
        weight4(t0, w);
#pragma unroll
        for (int l = 0; l < 4; l++)
            pos[l] = t0 + 1024 * l < ntiles ? atomicAdd(&s_hist[kOrderBins - 1 - min(w[l] >> 2, (uint32_t)(kOrderBins - 1))], 1u) : 0u;
#pragma unroll
        for (int l = 0; l < 4; l++)
            if (t0 + 1024 * l < ntiles) order[pos[l]] = (uint32_t)(t0 + 1024 * l);
    }
}

// exclusive scan of s[0 .. 1024) in place, one element per thread of the 1024-thread workgroup
__device__ __forceinline__ void scan1024(uint32_t* s, uint32_t* s_wsum /*[16]*/)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t v = s[tid];
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t n = __shfl_up(inc, d, 64);
        if (lane >= d) inc += n;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += s_wsum[w];
    __syncthreads();
    s[tid] = base + inc - v;
    __syncthreads();
}

// Mode 4 (see tile_for_block).  s_hist: [8][kOrderBins]; s_gw, s_gx: [kOrderMaxGroups].  All 1024 threads must call it.
// group_xcd [kOrderMaxGroups] (global): the group -> XCD map.  The forward (deal = true) deals the groups by list length and
// stores the map; the backward reuses it (its weights, the traversed lengths, follow the list lengths, and the records a
// group's tiles share should meet the L2 that already holds them): no second ranking.
__device__ __forceinline__ void tile_order_xcd_body(const uint2* ranges, const uint32_t* weights, int tiles_x, int tiles_y, uint32_t* order,
                                                    uint32_t* group_xcd, bool deal, uint32_t* s_hist, uint32_t* s_gw, uint32_t* s_gx,
                                                    uint32_t* s_wsum)
{
    const int tid = threadIdx.x;
    const int ntiles = tiles_x * tiles_y, gtx = (tiles_x + kOrderGroup - 1) / kOrderGroup, ngroups = order_groups(tiles_x, tiles_y);
    const int slots = order_slots(tiles_x, tiles_y);
    // a thread's tiles are tid, tid + 1024, ..: weight and group of the first kKeep stay in registers (800 x 800: 3 per thread)
    constexpr int kKeep = 4;
    uint32_t wk[kKeep], gk[kKeep];
    auto weight = [&](int t) { return weights ? weights[t] : (ranges[t].y - ranges[t].x); };
    auto group = [&](int t) { return (uint32_t)(((t / tiles_x) / kOrderGroup) * gtx + (t % tiles_x) / kOrderGroup); };
#pragma unroll
    for (int i = 0; i < kKeep; i++) {
        const int t = tid + 1024 * i;
        wk[i] = t < ntiles ? weight(t) : 0u;
        gk[i] = t < ntiles ? group(t) : 0u;
    }
    auto wt = [&](int i, int t) { return i < kKeep ? wk[i] : weight(t); };
    auto gr = [&](int i, int t) { return i < kKeep ? gk[i] : group(t); };
    s_gw[tid] = 0;
    for (int i = tid; i < 8 * kOrderBins; i += 1024) s_hist[i] = 0;
    for (int i = tid; i < slots; i += 1024) order[i] = (uint32_t)ntiles;   // empty slot
    if (!deal && tid < ngroups) s_gx[tid] = group_xcd[tid] & 7u;   // (& 7: a forward under another tile order left no map -- any map is valid)
    __syncthreads();
    if (deal) {
        for (int i = 0, t = tid; t < ntiles; i++, t += 1024) atomicAdd(&s_gw[gr(i, t)], wt(i, t));
        __syncthreads();
        // rank of every group by weight (descending; 64 entries per bin, ties in any order) -> its XCD in snake order
        const uint32_t gwt = tid < ngroups ? s_gw[tid] : 0u;
        const uint32_t gbin = kOrderBins - 1 - min(gwt >> 6, (uint32_t)(kOrderBins - 1));
        if (tid < ngroups) atomicAdd(&s_hist[gbin], 1u);
        __syncthreads();
        scan1024(s_hist, s_wsum);
        if (tid < ngroups) {
            const uint32_t r = atomicAdd(&s_hist[gbin], 1u);
            const uint32_t x = (r >> 3) & 1u ? 7u - (r & 7u) : (r & 7u);
            s_gx[tid] = x;
            group_xcd[tid] = x;
        }
        __syncthreads();
        s_hist[tid] = 0;
        __syncthreads();
    }
    // per XCD: counting sort of its tiles by weight, heaviest first
    for (int i = 0, t = tid; t < ntiles; i++, t += 1024) {
        const uint32_t bin = kOrderBins - 1 - min(wt(i, t) >> 2, (uint32_t)(kOrderBins - 1));
        atomicAdd(&s_hist[s_gx[gr(i, t)] * kOrderBins + bin], 1u);
    }
    __syncthreads();
    {   // the 8 exclusive scans at once: thread <-> bin, one shuffle network carrying 8 values
        const int lane = tid & 63, wave = tid >> 6;
        uint32_t v[8], inc[8];
#pragma unroll
        for (int x = 0; x < 8; x++) { v[x] = s_hist[x * kOrderBins + tid]; inc[x] = v[x]; }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const uint32_t n = __shfl_up(inc[x], d, 64);
                if (lane >= d) inc[x] += n;
            }
        if (lane == 63)
#pragma unroll
            for (int x = 0; x < 8; x++) s_gw[x * 16 + wave] = inc[x];   // the group weights are no longer needed
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 8; x++) {
            uint32_t base = 0;
            for (int w = 0; w < wave; w++) base += s_gw[x * 16 + w];
            s_hist[x * kOrderBins + tid] = base + inc[x] - v[x];
        }
        __syncthreads();
    }
    for (int i = 0, t = tid; t < ntiles; i++, t += 1024) {
        const uint32_t x = s_gx[gr(i, t)];
        const uint32_t bin = kOrderBins - 1 - min(wt(i, t) >> 2, (uint32_t)(kOrderBins - 1));
        const uint32_t pos = atomicAdd(&s_hist[x * kOrderBins + bin], 1u);
        order[8u * pos + x] = (uint32_t)t;
    }
}

__global__ void __launch_bounds__(1024) tile_order_kernel(const uint2* ranges, const uint32_t* weights, int tiles_x, int tiles_y, int mode,
                                                          uint32_t* order, uint32_t* group_xcd)
{
    __shared__ uint32_t s_hist[8 * kOrderBins];
    __shared__ uint32_t s_gw[kOrderMaxGroups], s_gx[kOrderMaxGroups];
    __shared__ uint32_t s_wsum[16];
    if (mode == 4) tile_order_xcd_body(ranges, weights, tiles_x, tiles_y, order, group_xcd, false, s_hist, s_gw, s_gx, s_wsum);
    else tile_order_body(ranges, weights, tiles_x * tiles_y, order, s_hist, s_wsum);
}

// The backward's two preparations as ONE launch: workgroups 0 .. n-2 clear the surfels' accumulator rows (what hipMemsetAsync did),
// the last one orders the tiles by the length the forward traversed (tile_order_kernel) -- the two were 7 + 6 us back to back in
// front of the backward blend of every step.
__global__ void __launch_bounds__(1024) prep_bwd_kernel(float4* __restrict__ acc, size_t n4, const uint32_t* weights, int tiles_x, int tiles_y, int mode,
                                                        uint32_t* order, uint32_t* group_xcd, uint32_t* long_thr /*[2]: [1] written here*/, uint32_t long_div,
                                                        const uint32_t* clean_flag /*1: the forward blend's rider zeroed the rows, or null*/)
{
    __shared__ uint32_t s_hist[8 * kOrderBins];
    __shared__ uint32_t s_gw[kOrderMaxGroups], s_gx[kOrderMaxGroups];
    __shared__ uint32_t s_wsum[16];
    if (blockIdx.x == gridDim.x - 1) {
        {   // long-tile path of the backward blend: a tile is long from 512 traversed entries and (sum of the traversed lengths) / long_div on
            const int ntiles = tiles_x * tiles_y;
            uint32_t sum = 0;
            for (int t0 = threadIdx.x; t0 < ntiles; t0 += 4096) {   // four loads in flight per trip (tile_order_body)
                uint32_t w[4];
#pragma unroll
                for (int l = 0; l < 4; l++) w[l] = t0 + 1024 * l < ntiles ? weights[t0 + 1024 * l] : 0u;
                sum += (w[0] + w[1]) + (w[2] + w[3]);
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
            if ((threadIdx.x & 63) == 0) s_wsum[threadIdx.x >> 6] = sum;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t tot = 0;
                for (int w = 0; w < 16; w++) tot += s_wsum[w];
                long_thr[1] = max(512u, tot / max(long_div, 1u));
            }
            __syncthreads();
        }
        if (mode == 4) tile_order_xcd_body(nullptr, weights, tiles_x, tiles_y, order, group_xcd, false, s_hist, s_gw, s_gx, s_wsum);
        else tile_order_body(nullptr, weights, tiles_x * tiles_y, order, s_hist, s_wsum);
        return;
    }
    if (clean_flag && *clean_flag == 1u) return;
    const size_t stride = (size_t)(gridDim.x - 1) * 1024;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < n4; i += stride) acc[i] = z;
}

}  // namespace dgs
