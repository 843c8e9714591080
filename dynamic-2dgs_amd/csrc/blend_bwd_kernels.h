// blend_bwd_kernels.h -- the per-tile backward alpha blend for gfx950: bwd_quadrant (one quadrant of a tile, back to front; also the
// long-tile path), blend_bwd_kernel with its three ways of summing per surfel (float atomics, per-entry rows, fixed point), and the
// two kernels that turn the deterministic variants' sums into accumulator rows.  The design the forward and the backward share is
// described in blend_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blend_common.h"
#include "surfel_math.h"
#include "wave_reduce.h"

namespace dgs {

struct BlendBwdArgs {
    const uint2* ranges;
    const uint32_t* order;
    const uint32_t* point_list;
    const float4* rec;
    int W, H, tiles_x, tiles_y, mode;
    const float* bg;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* tile_last;
    const float* dL_dpix;     // [3,H,W]
    const float* dL_dothers;  // [8,H,W]
    float* acc;               // [P, kAccFloats], zeroed
    float* det_part;          // deterministic variant 1 only: [num_rendered][4 waves][kAccFloats], zeroed (see det_reduce_kernel)
    unsigned long long* acc64; // deterministic variant 2 only: [P, kAccFloats] fixed-point sums (2^-44), zero on entry (fixed_to_acc_kernel)
    uint32_t* clean_flag;      // BlendFwdArgs::clean_flag: the accumulator rows are written from here on (or null)
    const LongThr* long_thr;  // thresholds of the long-tile path, or null (path off: grid = blend_grid_size)
};

// ---- wave reduction of the 16 per-surfel partials of one (wave, entry) visit --------------------------------------------
// Transposition through the wave's own LDS (wave_reduce.h: 16 ds_write_addtid_b32 + 4 ds_read_b128 + 17 VALU), in two rounds of
// 8 values through 2 KB per wave.  The four earlier implementations (butterfly on the LDS crossbar 0.338 ms, matrix pipe 0.548,
// permlane + MFMA hybrid 0.455, permlane + DPP 0.304-0.315; this one 0.267; one round of 16 values through 4 KB -- 3 workgroups
// per CU instead of 5 -- 0.304) and their measurements: DESIGN.md section 4.
// On return lane l with (l & 3) == 0 holds the wave total of v[(l >> 3) + 2 (l & 4)]; reduce16_slot() says so.
struct BwdRed { float v[8][64]; };   // one wave's transposition buffer
typedef RedLds BwdRedCtx;

__device__ __forceinline__ float wave_reduce16(float (&v)[16], int lane, const BwdRedCtx& rc) { return wave_reduce16_lds(v, rc, lane); }

// which of the 16 values lane `lane` holds after wave_reduce16, or -1 if the lane holds a duplicate
__device__ __forceinline__ int reduce16_slot(int lane) { return (lane & 3) == 0 ? (lane >> 3) + 2 * (lane & 4) : -1; }

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

constexpr int kDetRows = 4;   // rows of det_part per list entry: one per wave

#ifndef DGS_BWD_MINWAVES
#define DGS_BWD_MINWAVES 5
#endif
// DET = 0: the per-(wave, entry) sums go into the surfel's accumulator row with hardware float atomics (order of arrival:
// results differ at the rounding level from run to run, like the reference's).  DET = 1 (dgs_set_option(7, 1), tests): every
// (list entry, wave) owns a row of det_part and stores its sums there; det_reduce_kernel adds the rows of a surfel in a fixed order.
// DET = 2 (dgs_set_option(7, 2), round 5): the sums are added as 64-bit FIXED-POINT numbers (units of 2^-44, |sum| < 2^18) with
// integer atomics -- integer addition is associative, so the result does not depend on the order of arrival: bit-identical
// gradients from run to run at the speed of the default kernel, legal inside a captured graph (variant 1 is neither: it allocates
// per call and searches lists).  The price is the fixed quantum: a partial sum below 6e-14 is lost and one of 1e-9 keeps 4-5
// digits, where fp32 keeps 7 -- a different (slightly noisier) optimisation than the default, which is why it is an option:
// reproducible pre-fits (bench.py --workload trained, fit(deterministic=True)) and tests.
__device__ __forceinline__ unsigned long long to_fixed44(float v)
{
    v = fminf(fmaxf(v, -262144.0f), 262144.0f);
    return (unsigned long long)__float2ll_rn(v * 17592186044416.0f);   // 2^44; two's complement: unsigned wrap-around adds signed numbers
}

// 48 entries per chunk and DGS_BWD_MINWAVES 5 go together: 30 KB of LDS = 5 workgroups per CU, 0.267 ms at 200k / 800x800; 64 entries
// at 4 workgroups per CU: 0.281 -- the occupancy decides, the chunk size does not
#ifndef DGS_BWD_CHUNK
#define DGS_BWD_CHUNK 48
#endif
constexpr int kChunkB = DGS_BWD_CHUNK;   // list entries the backward stages per wave and step (lanes >= kChunkB stage nothing): sizes the slice
struct BwdStage {            // one wave's staging slice: the chunk's visited entries, compacted (+1: the visit loop reads one slot ahead)
    f32x4 a[3][kChunkB + 1];  // alpha part of the entry's affine image (tile_affine)
    f32x4 tw[kChunkB + 1];    // (Tw.x Tw.y Tw.z opacity)
    f32x4 tuv[kChunkB + 1];   // (Tu.x Tu.y Tv.x Tv.y): k.xy, l.xy of a pixel are rebuilt from them
    f32x4 q3[kChunkB + 1];    // (n.x n.y n.z r)
    f32x4 q4[kChunkB + 1];    // (g b, 0-based list index as bits, surfel id as bits)
};

// One quadrant of a tile, back to front.  LONG = false: the whole list behind the quadrant's last contributor, one wave (the kernel's
// normal path, q = wave).  LONG = true ("long tiles" in blend_common.h): the workgroup is ONE quadrant of a long tile and its
// wave `seg` takes the seg-th quarter of that range.  Both recurrences of the backward are linear in the state that enters a quarter --
// T <- T / (1 - alpha) and acc <- (1 - alpha) acc + alpha u, with alpha and u functions of the entry and the pixel only -- so pass 1
// walks the quarter once without the gradient arithmetic and leaves (F, A, B) per pixel: T_out = F T_in, acc_out = A acc_in + B; every
// wave then composes the quarters behind its own (they were walked by the other waves at the same time) and runs the real pass from
// the state that reaches it.  1.4 x the arithmetic on a quarter of the critical path; the gradients differ from the serial walk in
// rounding only (products and sums taken quarter-wise), like two runs of the atomic backward do.
template <int DET, bool LONG>
__device__ __forceinline__ void bwd_quadrant(const BlendBwdArgs& a, int tile, int q, int seg, BwdStage& S, const BwdRedCtx& rc, float* xfer /*LONG: [4][3][64]*/)
{
    const int ntiles = a.tiles_x * a.tiles_y;
    const int lane = threadIdx.x & 63;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    int lx_, ly_;
    lane_pixel(64 * q + lane, lx_, ly_);
    const int px = tx * kTileX + lx_, py = ty * kTileY + ly_;
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px + 0.5f, pfy = (float)py + 0.5f;
    const float tpx = (float)(tx * kTileX), tpy = (float)(ty * kTileY);
    const float X0 = tpx + 8.0f, Y0 = tpy + 8.0f;
    const float qx = tpx + (float)(8 * (q & 1)), qy = tpy + (float)(8 * (q >> 1));
    const float qus0 = kSqrt2 * ((q & 1) ? 0.5f : -7.5f), qvs0 = kSqrt2 * ((q & 2) ? 0.5f : -7.5f);
    const float us = kSqrt2 * ((float)lx_ - 7.5f), vs = kSqrt2 * ((float)ly_ - 7.5f);
    const uint2 range = a.ranges[tile];

    const size_t plane = (size_t)ntiles * kTilePix;
    const size_t slot_px = (size_t)tile * kTilePix + 64 * q + lane;
    PixBwdA st;
    {
        float gpix[3] = {0.f, 0.f, 0.f}, goth[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (inside) {
            const size_t HW = (size_t)a.H * a.W;
            const size_t pix = (size_t)py * a.W + px;
#pragma unroll
            for (int c = 0; c < 3; c++) gpix[c] = a.dL_dpix[c * HW + pix];
#pragma unroll
            for (int c = 0; c < 8; c++) goth[c] = a.dL_dothers[c * HW + pix];
        }
        const int last = inside ? (int)a.n_contrib[slot_px] : 0;
        const int medc = inside ? (int)a.n_contrib[plane + slot_px] : 0;
        // A pixel nothing contributed to never uses its gradient in the reference (backward.cu:283-300: the loop over its contributors is
        // empty), whatever that gradient is -- and PyTorch hands such pixels NaN: the reference's own render() divides the depth map by an
        // alpha of 0 there (gaussian_renderer/__init__.py:186-187; 0 / 0 in the division's backward).  Here the lanes of a visit multiply
        // before they mask, so the value must not be read at all.
        if (last == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) gpix[c] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; c++) goth[c] = 0.f;
        }
        pixbwd_init_affine(st, inside ? a.final_T[slot_px] : 0.f, a.final_T[plane + slot_px], a.final_T[2 * plane + slot_px], last, medc, gpix,
                           goth, a.bg);
    }
    // highest entry any lane of this wave needs: the wave walks the list back to front from there (backward.cu:276-279 skips the
    // entries behind a pixel's last contributor one by one)
    int wave_last = st.last_contributor;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        int o = __shfl_xor(wave_last, d, 64);
        wave_last = o > wave_last ? o : wave_last;
    }
    wave_last = __builtin_amdgcn_readfirstlane(wave_last);  // uniform by construction
    const int rslot = reduce16_slot(lane);
    // the range of list entries this wave walks: [lo, hi), back to front
    const int lo = LONG ? (int)(((long long)wave_last * seg) >> 2) : 0, hi = LONG ? (int)(((long long)wave_last * (seg + 1)) >> 2) : wave_last;
    float xF = 1.0f, xA = 1.0f, xB = 0.0f;   // pass 1 (LONG): the quarter's transfer of (T, acc)

    // chunk lane l holds list entry e = top - l; the entries that can touch the quadrant are compacted in that (back to front) order
    const bool stager = kChunkB == 64 || lane < kChunkB;
    auto walk = [&](auto light_tag) {
        constexpr bool kLight = decltype(light_tag)::value;
        uint32_t id_next = stager && hi - 1 - lane >= lo ? a.point_list[range.x + (uint32_t)(hi - 1 - lane)] : 0u;
        for (int top = hi - 1; top >= lo; top -= kChunkB) {
            const int e_mine = top - lane;
            const uint32_t id = id_next;   // (lanes beyond the front of the range hold id 0: a valid record, masked out below)
            // straight-line staging, see blend_fwd_rows_kernel
            const float4* src = a.rec + (size_t)id * kRecQuads;
            const float4 q0 = src[0], q1 = src[1], q2 = src[2], q3s = src[3], q4s = src[4], bx = src[5];
            id_next = stager && e_mine - kChunkB >= lo ? a.point_list[range.x + (uint32_t)(e_mine - kChunkB)] : 0u;
            const TileAffine ta = tile_affine(as_quad(q0), as_quad(q1), as_quad(q2), X0, Y0);
            const bool hit = stager & (e_mine >= lo) & block_box_hit(bx, qx, qy) & block_hit_affine(ta, qus0, qus0 + 7.0f * kSqrt2, qvs0, qvs0 + 7.0f * kSqrt2);
            const unsigned long long m = ballot64(hit);
            if (m == 0ull) continue;
            if (hit) {
                const int slot = lane_rank(m);
                S.a[0][slot] = mk4(ta.a0.x, ta.a0.y, ta.a0.z, ta.a0.w);
                S.a[1][slot] = mk4(ta.a1.x, ta.a1.y, ta.a1.z, ta.a1.w);
                S.a[2][slot] = mk4(ta.a2.x, ta.a2.y, ta.a2.z, ta.a2.w);
                S.tw[slot] = mk4(q1.z, q1.w, q2.x, q2.w);
                S.tuv[slot] = mk4(q0.x, q0.y, q0.w, q1.x);
                S.q3[slot] = mk4(q3s);
                S.q4[slot] = mk4(q4s.x, q4s.y, __int_as_float(e_mine), __uint_as_float(id));
            }
            __builtin_amdgcn_wave_barrier();   // the slice is private to this wave: its LDS writes above are ordered before its reads below
            const int nhit = __builtin_popcountll(m);
            f32x4 a0 = S.a[0][0], a1 = S.a[1][0], a2 = S.a[2][0];
            f32x4 tw = S.tw[0], tuv = S.tuv[0], q3 = S.q3[0], q4 = S.q4[0];
            for (int i = 0; i < nhit; i++) {
                AlphaEval ev;
                bool ok = alpha_affine(us, vs, as_quad(a0), as_quad(a1), as_quad(a2), ev);
                asm volatile("" : "+v"(ev.a), "+v"(ev.alpha) : : "memory");   // see blend_fwd_rows_kernel: one register set, loads pinned behind their last use
                a0 = S.a[0][i + 1]; a1 = S.a[1][i + 1]; a2 = S.a[2][i + 1];
                DGS_PIN4(a0); DGS_PIN4(a1); DGS_PIN4(a2);
                const int e = __builtin_amdgcn_readfirstlane(__float_as_int(q4.z));  // 0-based list index == the reference's `contributor`
                ok = ok & (e < st.last_contributor);
                if (ballot64(ok) != 0ull) {
                    bool use3d;
                    const float depth = alpha_depth(ev, tw.x, tw.y, tw.z, use3d);
                    ok = ok & (depth >= kNear);
                    if (kLight) {
                        // pass 1 of a long tile: only what the two recurrences need (pixbwd_step_affine's alpha, 1 / (1 - alpha) and u)
                        const float alpha = ok ? ev.alpha : 0.f;
                        const float u = pixbwd_u_affine(st, ok, depth, e, as_quad(q3), Quad{q4.x, q4.y, 0.f, 0.f});
                        xF = xF * fast_rcp(1.f - alpha);
                        xA = xA - alpha * xA;
                        xB = xB + alpha * (u - xB);
                    } else {
                    // every lane runs the step; a lane that does not blend the entry contributes exact zeros (pixbwd_step_affine)
                    float out[16], out2d[2];
                    pixbwd_step_affine(st, ev, ok, use3d, depth, e, pfx, pfy, tw.x, tw.y, as_quad(tuv), tw.w, as_quad(q3),
                                       Quad{q4.x, q4.y, 0.f, 0.f}, out, out2d);
                    // (two ballots of plain comparisons and scalar logic: ballot64(ok && !use3d) compiled to a select and a compare per visit)
                    const bool any2d = (ballot64(ok) & ~ballot64(use3d)) != 0ull;
                    // wave-uniform row address: keep it on the scalar unit (SGPR base + per-lane offset in the atomic)
                    const size_t row = DET == 1 ? ((size_t)(range.x + (uint32_t)e) * kDetRows + q) * kAccFloats
                                                : (size_t)__builtin_amdgcn_readfirstlane(__float_as_uint(q4.w)) * kAccFloats;
                    float* dst = (DET == 1 ? a.det_part : a.acc) + row;
                    unsigned long long* dst64 = DET == 2 ? a.acc64 + row : nullptr;
                    const float tot = wave_reduce16(out, lane, rc);
                    if (rslot >= 0) {
                        if (DET == 1) dst[rslot] = tot;
                        else if (DET == 2) atomicAdd(dst64 + rslot, to_fixed44(tot));
                        else atomicAdd(dst + rslot, tot);
                    }
                    if (any2d) {  // rare 2-D filter branch (backward.cu:436-443)
                        const float mx = wave_sum(out2d[0]);
                        const float my = wave_sum(out2d[1]);
                        if (lane == 0) {
                            if (DET == 1) { dst[kAccMean2D] = mx; dst[kAccMean2D + 1] = my; }
                            else if (DET == 2) { atomicAdd(dst64 + kAccMean2D, to_fixed44(mx)); atomicAdd(dst64 + kAccMean2D + 1, to_fixed44(my)); }
                            else { atomicAdd(dst + kAccMean2D, mx); atomicAdd(dst + kAccMean2D + 1, my); }
                        }
                    }
                    }
                }
                asm volatile("" : "+v"(st.T) : : "memory");
                tw = S.tw[i + 1]; tuv = S.tuv[i + 1]; q3 = S.q3[i + 1]; q4 = S.q4[i + 1];
                DGS_PIN4(tw); DGS_PIN4(tuv); DGS_PIN4(q3); DGS_PIN4(q4);
            }
            __builtin_amdgcn_wave_barrier();
        }
    };

    if (LONG) {
        walk(std::true_type{});
        xfer[(seg * 3 + 0) * 64 + lane] = xF;
        xfer[(seg * 3 + 1) * 64 + lane] = xA;
        xfer[(seg * 3 + 2) * 64 + lane] = xB;
        __syncthreads();
        // the state that reaches this quarter: (T_final, 0) through the quarters behind it, back to front
        float T = st.T, acc = 0.0f;
        for (int j = 3; j > seg; j--) {
            T = T * xfer[(j * 3 + 0) * 64 + lane];
            acc = xfer[(j * 3 + 1) * 64 + lane] * acc + xfer[(j * 3 + 2) * 64 + lane];
        }
        st.T = T;
        st.acc = acc;
        __syncthreads();   // xfer lives in the reduction buffers, which the real pass writes
    }
    walk(std::false_type{});
}

template <int DET>
__global__ void __launch_bounds__(kTilePix, DGS_BWD_MINWAVES) blend_bwd_kernel(BlendBwdArgs a)  // workgroups per CU = waves per SIMD the register allocator must allow
{
    __shared__ BwdStage s_stage[4];
    __shared__ BwdRed s_red[4];
    static_assert(sizeof(BwdRed) * 4 >= 4 * 3 * 64 * sizeof(float), "the long path's transfer table lives in the reduction buffers");

    const int ntiles = a.tiles_x * a.tiles_y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (a.clean_flag && blockIdx.x == 0 && threadIdx.x == 0) *a.clean_flag = 0u;   // (prep_bwd_kernel read it in the launch before)
    int tile, lq = -1;
    if (a.long_thr) {   // tile order 3 with the long-tile path (long_decode)
        if (!long_decode(blockIdx.x, a.order, ntiles, a.long_thr->bwd, a.tile_last, a.ranges, tile, lq)) return;
    } else {
        tile = tile_for_block(blockIdx.x, a.tiles_x, a.tiles_y, a.mode);
        if (a.mode < 3 && tile >= ntiles) return;
        if (a.mode >= 3) tile = (int)a.order[tile];
        if (tile >= ntiles) return;   // mode 4: empty slot
    }
    if (a.tile_last[tile] == 0u) return;   // no pixel of the tile blended anything
    BwdRedCtx rc;
    rc.init(&s_red[wave].v[0][0], lane);
    if (lq >= 0) {
        bwd_quadrant<DET, true>(a, tile, lq, wave, s_stage[wave], rc, &s_red[0].v[0][0]);
        return;
    }
    bwd_quadrant<DET, false>(a, tile, wave, 0, s_stage[wave], rc, nullptr);
}

// Deterministic variant 2: the fixed-point rows -> the float accumulator rows the per-surfel kernel reads; the fixed-point rows are
// left zeroed for the next backward.
__global__ void __launch_bounds__(256) fixed_to_acc_kernel(unsigned long long* __restrict__ acc64, float* __restrict__ acc, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long v = (long long)acc64[i];
    acc64[i] = 0ull;
    acc[i] = (float)((double)v * (1.0 / 17592186044416.0));
}

// Deterministic reduction of the backward blend (test option): one thread per surfel walks the tiles of its rectangle in
// row-major order, finds its entry in the tile's sorted list and adds the four waves' rows in order 0..3.  Same sums as the
// atomics in ONE fixed order: two runs give bit-identical gradients.  Slow by design (linear search of the lists).
__global__ void __launch_bounds__(256) det_reduce_kernel(int P, const int* radii, const uint2* rects, int tiles_x, const uint2* ranges,
                                                         const uint32_t* point_list, const float* part, float* acc)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P || !(radii[idx] > 0)) return;
    const uint2 r = rects[idx];
    const int x0 = (int)(r.x & 0xffffu), x1 = (int)(r.x >> 16), y0 = (int)(r.y & 0xffffu), y1 = (int)(r.y >> 16);
    float sum[kAccFloats];
#pragma unroll
    for (int k = 0; k < kAccFloats; k++) sum[k] = 0.f;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            const uint2 rg = ranges[y * tiles_x + x];
            for (uint32_t pos = rg.x; pos < rg.y; pos++) {
                if (point_list[pos] != (uint32_t)idx) continue;
                for (int w = 0; w < kDetRows; w++) {
                    const float* row = part + ((size_t)pos * kDetRows + w) * kAccFloats;
#pragma unroll
                    for (int k = 0; k < kAccFloats; k++) sum[k] += row[k];
                }
                break;
            }
        }
#pragma unroll
    for (int k = 0; k < kAccFloats; k++) acc[(size_t)idx * kAccFloats + k] = sum[k];
}

}  // namespace dgs
