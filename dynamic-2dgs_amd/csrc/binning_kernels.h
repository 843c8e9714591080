// binning_kernels.h -- from the surfels' tile rectangles to unsorted per-tile buckets of (depth, index) keys (gfx950): per-tile
// counts, the scan of the counts into tile ranges and bucket cursors (in one launch or three), the key scatter.
// Replaces cub InclusiveSum / duplicateWithKeys / identifyTileRanges of the reference (rasterizer_impl.cu:70-138, 278).
//
// Binning is a TILE-BUCKETED sort instead of the reference's global 44..46-bit LSD radix sort over
// (tile << 32 | depth) keys: count entries per tile (atomics), scan the T counts, scatter (depth, index) keys into
// the tile's bucket, then sort every bucket in LDS with one workgroup (tile_sort_kernels.h).  The global sort moves
// 12 B x R x ~12 through HBM; here every key is written once and read once, and tile ranges fall out of the scan.  The result
// is the same list: buckets ordered by tile, entries by (depth bits, surfel index) = the stable radix order.
#pragma once
#include <hip/hip_runtime.h>

#include "surfel_kernels.h"      // kSurfelBlock: the one-thread-per-surfel fallbacks are launched like the per-surfel kernels
#include "surfel_math.h"
#include "tile_order_kernels.h"  // the forward's dispatch order is written by the kernel that finishes the ranges

namespace dgs {

// ---- binning, step 1: per-tile entry counts -------------------------------------------------------------------
// kBinGroups workgroups each own a contiguous chunk of surfels and histogram its (surfel, tile) pairs in LDS
// (T counters: 10 KB at 800x800, 40 KB at 1600x1600); row g of the G x T matrix M receives the histogram.  Global
// atomics on 2500 hot counters measured 7.5 G/s on MI355X (1.5 M pairs = 200 us); LDS atomics make this ~20 us and
// the scatter below reuses the same chunking, so bucket positions need no global atomics either.
constexpr int kBinGroups = 256;
constexpr int kBinThreads = 1024;   // 16 waves per workgroup (one workgroup per CU): a chunk of ~782 surfels is ONE trip of the loop below instead of
                                    // three dependent ones (radii -> rectangle -> LDS atomics); count 12 -> 7, scatter 17 -> 14 us

#ifndef DGS_BIG_RECT
#define DGS_BIG_RECT 64
#endif
constexpr int kBigRect = DGS_BIG_RECT;   // tiles: a larger tile rectangle is walked by the whole wave instead of its own thread

struct BinArgs {
    int P, ntiles, tiles_x, chunk;   // chunk = surfels per workgroup
    const uint32_t* state;  // [3] num_rendered, longest, overflow (scatter is skipped when overflow is set)
    const int* radii;
    const uint2* rects;
    const float4* rec;
    uint32_t* M;            // [kBinGroups, T] counts, then bucket write cursors
    uint64_t* keys;         // [R] (scatter only)
    uint32_t* sync;         // count only: nsync words cleared for bin_offsets_kernel (its workgroups' aggregates and ticket), or null
    int nsync;
    // scatter only, rider (order != null): one more workgroup at the end of the grid clears tile_last and writes the forward blend's
    // dispatch order from the ranges -- next to the scatter instead of as the serial tail of bin_offsets_kernel's last workgroup
    const uint2* ranges; uint32_t* order; uint32_t* group_xcd; uint32_t* tile_last; int tiles_y, order_mode;
};

__global__ void __launch_bounds__(kBinThreads) count_tiles_lds_kernel(BinArgs a)
{
    extern __shared__ uint32_t s_hist[];
    const int g = blockIdx.x, tid = threadIdx.x;
    for (int t = tid; t < a.ntiles; t += kBinThreads) s_hist[t] = 0;
    if (g == 0 && a.sync)
        for (int i = tid; i < a.nsync; i += kBinThreads) a.sync[i] = 0u;
    __syncthreads();
    const int end = min(a.P, (g + 1) * a.chunk);
    const int lane = tid & 63;
    for (int base = g * a.chunk; base < end; base += kBinThreads) {   // (all threads of a wave take the trip together: wave-wide votes below)
        const int idx = base + tid;
        const bool vis = idx < end && a.radii[idx] > 0;
        const uint2 r = vis ? a.rects[idx] : make_uint2(0u, 0u);
        const int x0 = (int)(r.x & 0xffffu), x1 = (int)(r.x >> 16), y0 = (int)(r.y & 0xffffu), y1 = (int)(r.y >> 16);
        const int w = max(x1 - x0, 0), area = w * max(y1 - y0, 0);
        const bool big = area > kBigRect;
        if (!big)
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) atomicAdd(&s_hist[y * a.tiles_x + x], 1u);
        // (more than 64 tiles: below that the lanes of the wave would idle, and on the uniform scene the vote alone costs 1 us)
        // a rectangle of hundreds of tiles in ONE thread's loop is what the other 63 lanes wait for (a densified scene keeps a few
        // screen-filling splats: count 36 us / scatter 43 us for a third of the uniform scene's pairs): the wave walks it together
        unsigned long long todo = __ballot(big);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int X0 = __builtin_amdgcn_readlane(x0, src), Y0 = __builtin_amdgcn_readlane(y0, src);
            const int Wd = __builtin_amdgcn_readlane(w, src), n = __builtin_amdgcn_readlane(area, src);
            const float inv_w = __frcp_rn((float)Wd);
            for (int t = lane; t < n; t += 64) {
                const int row = (int)(((float)t + 0.5f) * inv_w);   // t / Wd without the integer division (t < 2^16, Wd <= 2^8: exact)
                atomicAdd(&s_hist[(Y0 + row) * a.tiles_x + X0 + (t - row * Wd)], 1u);
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < a.ntiles; t += kBinThreads) a.M[(size_t)g * a.ntiles + t] = s_hist[t];
}

// Column pass over M.  Block = 64 tiles x kColGroups row groups (kBinGroups / kColGroups rows per thread, all loads
// independent and in flight together); the partial sums of a tile meet in LDS.  The grid is only T / 64 workgroups, so the
// parallelism has to come from inside the workgroup: 16 groups of 16 rows (1024 threads) instead of 4 of 64.
//   counts == nullptr : M[g][t] <- ranges[t].x + sum_{g' < g} M[g'][t]   (where workgroup g starts writing tile t)
//   counts != nullptr : counts[t] = sum_g M[g][t]
constexpr int kColGroups = 16;
__global__ void __launch_bounds__(64 * kColGroups) column_pass_kernel(uint32_t* M, int ntiles, const uint2* ranges, uint32_t* counts)
{
    constexpr int kRows = kBinGroups / kColGroups;
    __shared__ uint32_t s_part[kColGroups][64];
    const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tx;
    uint32_t v[kRows];
    uint32_t sum = 0;
    if (t < ntiles) {
#pragma unroll
        for (int i = 0; i < kRows; i++) v[i] = M[(size_t)(ry * kRows + i) * ntiles + t];
#pragma unroll
        for (int i = 0; i < kRows; i++) sum += v[i];
    }
    s_part[ry][tx] = sum;
    __syncthreads();
    if (t >= ntiles) return;
    if (counts) {
        if (ry == 0) {
            uint32_t tot = 0;
#pragma unroll
            for (int r = 0; r < kColGroups; r++) tot += s_part[r][tx];
            counts[t] = tot;
        }
        return;
    }
    uint32_t run = ranges[t].x;
    for (int r = 0; r < ry; r++) run += s_part[r][tx];
#pragma unroll
    for (int i = 0; i < kRows; i++) {
        M[(size_t)(ry * kRows + i) * ntiles + t] = run;
        run += v[i];
    }
}

// duplicateWithKeys (rasterizer_impl.cu:70-111) for the tile-bucketed sort: the tile id is implied by the bucket, so
// the key only carries (depth, surfel index) -- the tie-break order of the reference's stable radix sort.
constexpr size_t kScatterRiderLds = (8 * kOrderBins + 2 * kOrderMaxGroups + 16) * sizeof(uint32_t);   // the rider workgroup's tables (below)
__global__ void __launch_bounds__(kBinThreads) scatter_keys_lds_kernel(BinArgs a)
{
    extern __shared__ uint32_t s_cur[];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (g == kBinGroups) {   // the rider (BinArgs::order); runs on an overflowed frame as well (its ranges are empty, the order still has to exist)
        // its tables live in the DYNAMIC buffer (the rider never uses the cursors; the host sizes the buffer for whichever is larger,
        // kScatterRiderLds): static arrays here would add 40 KB to every workgroup of the launch and push a 3840 x 2160 image
        // (32 400 tiles = 127 KB of cursors) past the 160 KB a workgroup can have
        uint32_t* s_hist = s_cur;
        uint32_t* s_gw = s_hist + 8 * kOrderBins;
        uint32_t* s_gx = s_gw + kOrderMaxGroups;
        uint32_t* s_osum = s_gx + kOrderMaxGroups;
        for (int i = tid; i < a.ntiles; i += kBinThreads) a.tile_last[i] = 0u;
        if (a.order_mode == 4) tile_order_xcd_body(a.ranges, nullptr, a.tiles_x, a.tiles_y, a.order, a.group_xcd, true, s_hist, s_gw, s_gx, s_osum);
        else tile_order_body(a.ranges, nullptr, a.ntiles, a.order, s_hist, s_osum);
        return;
    }
    if (a.state[2] != 0u) return;  // capacity overflow: nothing may be written
    for (int t0 = tid; t0 < a.ntiles; t0 += 4 * kBinThreads) {   // four loads in flight per trip (2500 tiles: one trip)
        uint32_t c[4];
#pragma unroll
        for (int l = 0; l < 4; l++) { const int t = t0 + l * kBinThreads; c[l] = t < a.ntiles ? a.M[(size_t)g * a.ntiles + t] : 0u; }
#pragma unroll
        for (int l = 0; l < 4; l++) { const int t = t0 + l * kBinThreads; if (t < a.ntiles) s_cur[t] = c[l]; }
    }
    __syncthreads();
    const int end = min(a.P, (g + 1) * a.chunk);
    const int lane = tid & 63;
    for (int base = g * a.chunk; base < end; base += kBinThreads) {
        const int idx = base + tid;
        const bool vis = idx < end && a.radii[idx] > 0;
        const uint2 r = vis ? a.rects[idx] : make_uint2(0u, 0u);
        const int x0 = (int)(r.x & 0xffffu), x1 = (int)(r.x >> 16), y0 = (int)(r.y & 0xffffu), y1 = (int)(r.y >> 16);
        const int w = max(x1 - x0, 0), area = w * max(y1 - y0, 0);
        const uint32_t depth = area > 0 ? __float_as_uint(a.rec[(size_t)idx * kRecQuads + 4].z) : 0u;
        const uint64_t key = ((uint64_t)depth << 32) | (uint32_t)idx;
        const bool big = area > kBigRect;
        if (!big)
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) a.keys[atomicAdd(&s_cur[y * a.tiles_x + x], 1u)] = key;
        unsigned long long todo = __ballot(big);   // large rectangles: the wave walks them together (count_tiles_lds_kernel)
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int X0 = __builtin_amdgcn_readlane(x0, src), Y0 = __builtin_amdgcn_readlane(y0, src);
            const int Wd = __builtin_amdgcn_readlane(w, src), n = __builtin_amdgcn_readlane(area, src);
            const uint64_t k = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)depth, src) << 32) | (uint32_t)__builtin_amdgcn_readlane(idx, src);
            const float inv_w = __frcp_rn((float)Wd);
            for (int t = lane; t < n; t += 64) {
                const int row = (int)(((float)t + 0.5f) * inv_w);
                a.keys[atomicAdd(&s_cur[(Y0 + row) * a.tiles_x + X0 + (t - row * Wd)], 1u)] = k;
            }
        }
    }
}

// Fallback for images with more tiles than fit the LDS histogram (> ~36k tiles): global atomics.
__global__ void __launch_bounds__(kSurfelBlock) count_tiles_global_kernel(int P, const int* radii, const uint2* rects, int tiles_x,
                                                                          uint32_t* tile_counts)
{
    const int idx = blockIdx.x * kSurfelBlock + threadIdx.x;
    if (idx >= P || !(radii[idx] > 0)) return;
    const uint2 r = rects[idx];
    const int x0 = (int)(r.x & 0xffffu), x1 = (int)(r.x >> 16), y0 = (int)(r.y & 0xffffu), y1 = (int)(r.y >> 16);
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) atomicAdd(&tile_counts[y * tiles_x + x], 1u);
}

// What is OR-ed into the overflow flag (dgs_set_overflow_flag): bit 0 the lists do not fit the capacity, bit 1 a list is longer than
// promised (option 6), bit 2 that list is longer than the segmented sort reaches (kSegCap * kMaxSegs) -- the caller picks its next
// configuration from the bits instead of trying the tiers one skipped step at a time.
__device__ __forceinline__ int overflow_reason(uint32_t total, uint32_t cap, uint32_t longest, uint32_t list_hint)
{
    int r = total > cap ? 1 : 0;
    if (list_hint > 0 && longest > list_hint) r |= longest > 57344u ? 6 : 2;
    return r;
}

// Exclusive scan of the per-tile counts (T = 2500 at 800x800, 10000 at 1600x1600) by ONE workgroup:
// ranges[t] = [start, end) (identifyTileRanges, rasterizer_impl.cu:116-138), cursor[t] = start (scatter cursors),
// *total_out = num_rendered (rasterizer_impl.cu:281).
// `cap` > 0 (capacity mode, no host round trip): if the lists do not fit the pre-sized binning buffer every tile is
// left empty (the frame renders as background) and *overflow is raised instead of writing out of bounds.
__global__ void __launch_bounds__(1024) scan_tiles_kernel(const uint32_t* counts, int ntiles, uint2* ranges, uint32_t* cursor,
                                                          uint32_t* total_out /*[3]: num_rendered, longest list, overflow*/,
                                                          uint32_t cap, int* overflow, uint32_t* order /*or null*/, uint32_t list_hint,
                                                          int tiles_x, int tiles_y, int order_mode, uint32_t* group_xcd,
                                                          uint32_t* tile_last /*[T]: zeroed here*/, uint32_t* long_thr /*[2]: [0] written here*/, uint32_t long_div)
{
    __shared__ uint32_t s_wsum[4], s_wmax[4];
    // the forward blend writes the per-tile maximum of the last contributor with atomicMax (a long tile is four workgroups)
    for (int t = threadIdx.x; t < ntiles; t += 1024) tile_last[t] = 0u;
    __shared__ uint32_t s_hist[8 * kOrderBins];
    __shared__ uint32_t s_gw[kOrderMaxGroups], s_gx[kOrderMaxGroups];
    __shared__ uint32_t s_osum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 256) {   // the scan proper: 256 threads, `per` consecutive tiles each
        const int per = (ntiles + 255) / 256;
        const int t0 = tid * per, t1 = min(ntiles, t0 + per);
        uint32_t sum = 0, mx = 0;
        for (int t = t0; t < t1; t++) { const uint32_t c = counts[t]; sum += c; mx = max(mx, c); }
        uint32_t inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t n = __shfl_up(inc, d, 64);
            if (lane >= d) inc += n;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if (lane == 63) s_wsum[wave] = inc;
        if (lane == 0) s_wmax[wave] = mx;
        s_hist[tid] = inc - sum;   // exclusive prefix inside the wave, parked for after the barrier
    }
    __syncthreads();
    if (tid < 256) {
        const int per = (ntiles + 255) / 256;
        const int t0 = tid * per, t1 = min(ntiles, t0 + per);
        const uint32_t total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        const uint32_t longest = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));
        // capacity mode: the lists must fit the pre-sized buffer, and -- if the caller promised a longest list (list_hint:
        // only the sort kernels for lists up to it were launched) -- no list may be longer than promised
        const bool over = cap > 0 && (total > cap || (list_hint > 0 && longest > list_hint));
        uint32_t run = s_hist[tid];
        for (int w = 0; w < wave; w++) run += s_wsum[w];
        for (int t = t0; t < t1; t++) {
            const uint32_t c = over ? 0u : counts[t];
            if (over) run = 0;
            ranges[t] = make_uint2(run, run + c);
            if (cursor) cursor[t] = run;
            run += c;
        }
        if (tid == 0) {
            total_out[0] = total;
            total_out[1] = longest;
            total_out[2] = over ? 1u : 0u;
            if (over && overflow) atomicOr(overflow, overflow_reason(total, cap, longest, list_hint));
            // long-tile path of the forward blend (blend_common.h): worth its extra arithmetic only where ONE tile's serial walk is as
            // long as the whole launch's throughput-bound time -- a list is long from 768 entries and num_rendered / long_div on
            long_thr[0] = max(768u, total / max(long_div, 1u));
        }
    }
    if (order) {
        // dispatch order of the forward blend (longest list first, tile_order_kernels.h): the ranges were just written by this
        // workgroup, visible to all of its threads after the fence + barrier
        __threadfence_block();
        __syncthreads();
        if (order_mode == 4) tile_order_xcd_body(ranges, nullptr, tiles_x, tiles_y, order, group_xcd, true, s_hist, s_gw, s_gx, s_osum);
        else tile_order_body(ranges, nullptr, ntiles, order, s_hist, s_osum);
    }
}

// Column sums, scan of the tile counts, bucket cursors and the forward's dispatch order in ONE launch (LDS-histogram path): replaces
// column_pass(counts) + scan_tiles + column_pass(cursors), three dependent launches of 5 + 10 + 5 us, each mostly launch and memory
// latency.  Workgroup b = 64 tiles x all kBinGroups rows of M, as in column_pass_kernel; its 64 tile counts are scanned by its
// first wave and the offset of the block is the sum of the aggregates of the workgroups before it, which every workgroup
// publishes (flag in the top bit) the moment it has it -- a one-level decoupled look-back: nobody waits for anything but
// lower-numbered workgroups, which are dispatched first.  The rows of M were read once and are rewritten from registers.
// The workgroup that finishes LAST (ticket) does what needs every range: num_rendered, the longest list, the capacity
// check (on overflow it clears all ranges again), tile_last, long_thr[0] and the dispatch order of the forward blend.
// sync: [2 nb + 1] words, zero on entry (count_tiles_lds_kernel clears them): aggregates, maxima, ticket.
struct OffsetsArgs {
    uint32_t* M; int ntiles; uint2* ranges;
    uint32_t* state;        // [3]: num_rendered, longest list, overflow
    uint32_t cap; int* overflow; uint32_t list_hint;
    uint32_t* order;        // or null
    int tiles_x, tiles_y, order_mode;
    uint32_t* group_xcd; uint32_t* tile_last; uint32_t* long_thr; uint32_t long_div;
    uint32_t* sync;
    int order_later;        // tile_last and the dispatch order are left to the scatter launch's rider workgroup (capacity mode: it always runs)
};

__global__ void __launch_bounds__(64 * kColGroups) bin_offsets_kernel(OffsetsArgs a)
{
    constexpr int kRows = kBinGroups / kColGroups;
    constexpr uint32_t kFlag = 0x80000000u;
    __shared__ uint32_t s_part[kColGroups][64];
    __shared__ uint32_t s_start[64];
    __shared__ uint32_t s_last;
    __shared__ uint32_t s_hist[8 * kOrderBins];
    __shared__ uint32_t s_gw[kOrderMaxGroups], s_gx[kOrderMaxGroups];
    __shared__ uint32_t s_osum[16];
    const int tid = threadIdx.x, tx = tid & 63, ry = tid >> 6;
    const int b = blockIdx.x, nb = gridDim.x;
    const int t = b * 64 + tx;
    uint32_t* const agg = a.sync;
    uint32_t* const amax = a.sync + nb;
    uint32_t* const ticket = a.sync + 2 * nb;
    uint32_t v[kRows];
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < kRows; i++) v[i] = 0;
    if (t < a.ntiles) {
#pragma unroll
        for (int i = 0; i < kRows; i++) v[i] = a.M[(size_t)(ry * kRows + i) * a.ntiles + t];
#pragma unroll
        for (int i = 0; i < kRows; i++) sum += v[i];
    }
    s_part[ry][tx] = sum;
    __syncthreads();
    if (ry == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int r = 0; r < kColGroups; r++) c += s_part[r][tx];
        uint32_t inc = c, mx = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t n = __shfl_up(inc, d, 64);
            if (tx >= d) inc += n;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if (tx == 63) {
            __hip_atomic_store(&amax[b], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&agg[b], kFlag | inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        uint32_t before = 0;
        for (int j = tx; j < b; j += 64) {
            uint32_t w = __hip_atomic_load(&agg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (!(w & kFlag)) {
                __builtin_amdgcn_s_sleep(1);
                w = __hip_atomic_load(&agg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            before += w & ~kFlag;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) before += (uint32_t)__shfl_xor((int)before, d, 64);
        const uint32_t start = before + inc - c;
        s_start[tx] = start;
        if (t < a.ntiles) a.ranges[t] = make_uint2(start, start + c);
    }
    __syncthreads();
    if (t < a.ntiles) {
        uint32_t run = s_start[tx];
        for (int r = 0; r < ry; r++) run += s_part[r][tx];
#pragma unroll
        for (int i = 0; i < kRows; i++) {
            a.M[(size_t)(ry * kRows + i) * a.ntiles + t] = run;
            run += v[i];
        }
    }
    // ticket: the ranges of this workgroup are released before it, the last one acquires everybody's.  ONE thread fences (behind the
    // barrier that completes the workgroup's stores): an agent-scope fence writes back / invalidates the XCD's L2, and 1024 threads
    // x 40 workgroups doing that made this kernel 39 us instead of 12
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(nb - 1);
        if (last) __threadfence();
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    uint32_t tot = 0, lng = 0;
    for (int j = tid; j < nb; j += 64 * kColGroups) {
        tot += __hip_atomic_load(&agg[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~kFlag;
        lng = max(lng, __hip_atomic_load(&amax[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        tot += (uint32_t)__shfl_xor((int)tot, d, 64);
        lng = max(lng, (uint32_t)__shfl_xor((int)lng, d, 64));
    }
    if (tx == 0) { s_part[0][ry] = tot; s_part[1][ry] = lng; }
    __syncthreads();
    uint32_t total = 0, longest = 0;
#pragma unroll
    for (int r = 0; r < kColGroups; r++) { total += s_part[0][r]; longest = max(longest, s_part[1][r]); }
    // capacity mode: the lists must fit the pre-sized buffer, and -- if the caller promised a longest list (list_hint: only the
    // sort kernels for lists up to it were launched) -- no list may be longer than promised (scan_tiles_kernel)
    const bool over = a.cap > 0 && (total > a.cap || (a.list_hint > 0 && longest > a.list_hint));
    if (over)
        for (int i = tid; i < a.ntiles; i += 64 * kColGroups) a.ranges[i] = make_uint2(0u, 0u);
    if (!a.order_later)
        for (int i = tid; i < a.ntiles; i += 64 * kColGroups) a.tile_last[i] = 0u;
    if (tid == 0) {
        a.state[0] = total;
        a.state[1] = longest;
        a.state[2] = over ? 1u : 0u;
        if (over && a.overflow) atomicOr(a.overflow, overflow_reason(total, a.cap, longest, a.list_hint));
        a.long_thr[0] = max(768u, total / max(a.long_div, 1u));
    }
    if (a.order && !a.order_later) {
        __threadfence_block();
        __syncthreads();
        if (a.order_mode == 4) tile_order_xcd_body(a.ranges, nullptr, a.tiles_x, a.tiles_y, a.order, a.group_xcd, true, s_hist, s_gw, s_gx, s_osum);
        else tile_order_body(a.ranges, nullptr, a.ntiles, a.order, s_hist, s_osum);
    }
}

struct ScatterArgs {
    int P;
    const int* radii;
    const float4* rec;
    const uint2* rects;
    const uint32_t* state;  // [3] num_rendered, longest, overflow
    uint32_t* cursor;       // [T] running write position of every tile bucket
    uint64_t* keys;         // [R] out: depth bits << 32 | surfel index, bucketed by tile (unordered inside a bucket)
    int tiles_x;
};

// global-atomics variant of scatter_keys_lds_kernel (fallback for very large tile counts)
__global__ void __launch_bounds__(kSurfelBlock) scatter_keys_kernel(ScatterArgs a)
{
    const int idx = blockIdx.x * kSurfelBlock + threadIdx.x;
    if (idx >= a.P || !(a.radii[idx] > 0) || a.state[2] != 0u) return;
    const uint2 r = a.rects[idx];
    const int x0 = (int)(r.x & 0xffffu), x1 = (int)(r.x >> 16), y0 = (int)(r.y & 0xffffu), y1 = (int)(r.y >> 16);
    if (x1 <= x0 || y1 <= y0) return;
    const uint64_t key = ((uint64_t)__float_as_uint(a.rec[(size_t)idx * kRecQuads + 4].z) << 32) | (uint32_t)idx;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            const uint32_t pos = atomicAdd(&a.cursor[y * a.tiles_x + x], 1u);
            a.keys[pos] = key;
        }
}

}  // namespace dgs
