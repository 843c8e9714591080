// blend_common.h -- what the per-tile forward and backward alpha blend for gfx950 share (blend_fwd_kernels.h, blend_bwd_kernels.h):
// vector and ballot helpers, the blockIdx -> tile maps of the tile orders, the long-tile dispatch.
//
// One 16x16 screen tile per 256-thread workgroup = 4 wave64; wave w owns the 8x8 pixel quadrant (w & 1, w >> 1) of the
// tile (surfel_math.h lane_pixel), so all 64 lanes of a wave consume the same staged surfel at the same time.
//
// The four waves of a tile run AUTONOMOUSLY: each walks the tile's depth-sorted list in chunks of 64 entries, one
// entry per lane.  The lane gathers the entry's packed 96-B record, turns it into the entry's AFFINE image for this tile
// (surfel_math.h tile_affine: p = A + dxs B + dys C around the projected centre -- 6 FMAs per pixel instead of 12 operations),
// tests it against the wave's own quadrant (exact pixel box of the record, then the exact footprint: block_hit_affine) and, if it
// can touch the quadrant, stages it in the WAVE'S OWN slice of LDS: three float4 planes for the alpha test, then Tw, normal and
// colour planes that are only read when some pixel blends the entry.  One ballot gives the chunk's 64-bit visit mask; the inner
// loop walks its set bits and reads the planes with wave-uniform addresses (LDS broadcast, conflict free).  No workgroup barrier
// inside the list loop: with the shared 256-entry batches of rounds 1-2 a wave spent 30-40 % of its cycles parked at the two
// barriers per batch waiting for its three siblings (SQ_WAIT_ANY, profiles/r02_pmc_blend_metric.json), and a tile ran as long
// as its slowest quadrant TWICE over (once per barrier).  The price: a record is fetched and its affine image computed by up to
// four waves instead of one (staging is ~100 VALU instructions per 64 entries against ~1300 for their visits).
// Replaces renderCUDA of forward.cu:265-463 and backward.cu:143-449.
#pragma once
#include <hip/hip_runtime.h>

#include "surfel_math.h"
#include "tile_order_kernels.h"

namespace dgs {

// ---- tunables ----------------------------------------------------------------------------------------------------------------
// What is left to the command line are values, not code paths: DGS_FWD_MINWAVES (blend_fwd_kernels.h), DGS_BWD_MINWAVES and
// DGS_BWD_CHUNK (blend_bwd_kernels.h), each with its measurement where it is defined (tools/ab_variants.sh builds twins with other values next to the product,
// tools/ab_check.sh runs the parity file and the timing on each).  The kernels and reductions that lost their measurement -- the
// one-list-per-wave forward, the row-per-block backward, four earlier wave reductions -- are in the git history; what retired each
// is the table of DESIGN.md section 4.
constexpr int kChunk = 64;   // list entries staged per wave and step: one per lane

__device__ __forceinline__ Quad as_quad(const float4& v) { return Quad{v.x, v.y, v.z, v.w}; }

// Staged planes are read as native 4-vectors and pinned as such (an empty asm that takes the whole vector): the loop-carried
// float4 of a software-pipelined read is otherwise split by the compiler into four ds_read_b32 with an address register each.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Quad as_quad(const f32x4& v) { return Quad{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ f32x4 mk4(float x, float y, float z, float w) { return f32x4{x, y, z, w}; }
__device__ __forceinline__ f32x4 mk4(const float4& v) { return f32x4{v.x, v.y, v.z, v.w}; }
#define DGS_PIN4(v) asm volatile("" : "+v"(v))

// __ballot() takes an int: the bool -> int -> "!= 0" round trip is not always folded back (a v_cndmask 0/1 + v_cmp_ne per use in the
// blend loops when the predicate is an AND of lane masks); the builtin takes the i1 as it is
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ unsigned long long wave_uniform_u64(unsigned long long v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

struct LongThr { uint32_t fwd, bwd; };   // long-tile path: thresholds of this launch (list length / traversed length), in the image buffer

// Tile order.  The dispatcher places workgroup b on XCD b % 8 (MI355X_MICROARCH.md) and every XCD has a private
// 4 MiB L2, so which tiles share an XCD decides how often a surfel record is re-fetched.  Modes (A/B-able at
// run time through dgs_set_option(DGS_OPT_TILE_ORDER, m)):
//   0  plain row-major blockIdx (neighbouring tiles land on 8 different L2s),
//   1  contiguous: XCD x gets tiles [x*T/8, (x+1)*T/8)  (best locality, but whole image bands -- empty sky vs
//      dense centre -- go to one XCD: load imbalance),
//   2  row-interleaved: XCD x gets tile rows r with r % 8 == x, walked left to right (horizontal neighbours
//      share an L2, every XCD samples the whole image height).
//   4  XCD-local groups, longest first inside an XCD: the image is cut into 4 x 4-tile groups (a surfel's tiles mostly fall
//      into one), the groups are dealt to the 8 XCDs heaviest-first in snake order (balanced sums), and XCD x walks ITS
//      tiles in descending length: order[8 k + x] = its k-th tile (tile_order_body; empty slots hold `ntiles`).
__device__ __forceinline__ int tile_for_block(int bid, int tiles_x, int tiles_y, int mode)
{
    constexpr int kXcd = 8;
    const int ntiles = tiles_x * tiles_y;
    if (mode == 0 || mode >= 3) return bid;  // modes 3, 4 index the sorted order[] with it
    const int xcd = bid % kXcd, k = bid / kXcd;
    if (mode == 1) {
        const int per = (ntiles + kXcd - 1) / kXcd;
        return xcd * per + k;  // may be >= ntiles for the padded tail; caller checks
    }
    // mode 2: the k-th tile of this XCD is in its (k / tiles_x)-th row
    const int row = (k / tiles_x) * kXcd + xcd;
    if (row >= tiles_y) return ntiles;
    return row * tiles_x + (k % tiles_x);
}

// grid size that covers every tile under `mode`
inline int blend_grid_size(int tiles_x, int tiles_y, int mode)
{
    const int ntiles = tiles_x * tiles_y;
    if (mode == 0 || mode == 3) return ntiles;
    if (mode == 4) return order_slots(tiles_x, tiles_y);
    if (mode == 1) return ((ntiles + 7) / 8) * 8;
    return ((tiles_y + 7) / 8) * tiles_x * 8;
}

// What the instruction mix of the blend kernels' visit loops costs on gfx950 (tools/micro/valu_issue_bench, profiles/r03_valu_issue_gfx950.txt):
// FMA / mul / add with VGPR operands 2.5 cycles per wave, anything with an SGPR operand, comparisons, min/max, selects 4.4-4.8,
// v_rcp / v_exp 8.5-12.7, and every scalar instruction takes one of the CU's ~1 per cycle scalar issue slots.  So the visit is
// built from plain FMAs on VGPR operands (entry constants arrive through LDS broadcasts, not SGPRs), one comparison decides the
// alpha test (alpha_affine), finished and outside pixels are poisoned with NaN coordinates instead of being masked, and the
// median bookkeeping is skipped once no pixel of the wave has T > 0.5.
// does the record's exact pixel box (q5) reach a pixel centre of the 8x8 block whose first pixel is (qx, qy)?
__device__ __forceinline__ bool block_box_hit(const float4& bx, float qx, float qy)
{
    return (bx.y >= qx + 0.5f) & (bx.x <= qx + 7.5f) & (bx.w >= qy + 0.5f) & (bx.z <= qy + 7.5f);
}

// slot of this lane among the set bits of m (number of set bits below the lane)
__device__ __forceinline__ int lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---- long tiles -------------------------------------------------------------------------------------------------------------
// A tile is one workgroup and a quadrant one wave that walks the tile's list serially, so a launch is never shorter than its longest
// list -- and a lone wave issues one instruction per ~8 cycles however much of the device is idle: on a densified scene, whose few
// covered tiles hold lists of 1-2 k entries, the heaviest tile alone was the launch.  The `kLongSlots` tiles at
// the head of the longest-first dispatch order whose length exceeds a per-launch threshold (long_thr: written next to the order by the
// kernel that sorts it) therefore get FOUR workgroups, one per quadrant, whose four waves share the list: both recurrences of the
// backward and the forward's T <- T - alpha T are linear in the state that enters a stretch of the list, so a stretch can be walked
// before that state is known (a light pass leaves the stretch's transfer per pixel), the transfers are composed, and the real pass
// starts from the state that reaches the stretch.  Backward: quarters of the traversed range (bwd_quadrant<.., LONG = true>); forward:
// rounds of four chunks, which end where the serial walk ends (blend_fwd_long).  1.4-1.5 x the arithmetic on a quarter of the critical
// path.  What differs from the serial walk is rounding (products and sums taken stretch-wise); the results are deterministic.
// Grid (tile order 3 only): blocks [0, 4 kLongSlots) = (slot, quadrant) pairs, quadrant-major -- a short tile in one of these slots is
// rendered by its quadrant-0 block, the other three exit --, blocks behind them the remaining slots of the order.
constexpr int kLongSlots = 256;

// blockIdx -> (tile, quadrant of a long tile or -1).  Returns false when the block has nothing to do.
__device__ __forceinline__ bool long_decode(int bid, const uint32_t* order, int ntiles, uint32_t thr, const uint32_t* lengths /*[T] or null*/,
                                            const uint2* ranges, int& tile, int& lq)
{
    lq = -1;
    if (bid >= 4 * kLongSlots) {
        const int slot = bid - 3 * kLongSlots;
        if (slot >= ntiles) return false;
        tile = (int)order[slot];
        return tile < ntiles;
    }
    // (slot, quadrant) = (bid % kLongSlots, bid / kLongSlots): the quadrant-0 blocks -- all a short tile needs -- are the first kLongSlots
    // blocks of the launch, in order, spread over the 8 XCDs like any other run of blocks (bid >> 2 / bid & 3 put every one of them
    // on XCD 0 or 4: +28 % on the uniform scene)
    const int slot = bid % kLongSlots, sub = bid / kLongSlots;
    if (slot >= ntiles) return false;
    tile = (int)order[slot];
    if (tile >= ntiles) return false;
    const uint32_t len = lengths ? lengths[tile] : ranges[tile].y - ranges[tile].x;
    if (len > thr) { lq = sub; return true; }
    return sub == 0;
}

inline int long_grid_size(int ntiles) { return ntiles + 3 * kLongSlots; }

}  // namespace dgs
