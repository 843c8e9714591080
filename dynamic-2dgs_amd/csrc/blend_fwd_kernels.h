// blend_fwd_kernels.h -- the per-tile forward alpha blend for gfx950: blend_fwd_rows_kernel (one list per 16-lane row of a wave)
// and its long-tile path blend_fwd_long (one quadrant of a long tile per workgroup).  The design the forward and the backward
// share is described in blend_common.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "blend_common.h"
#include "surfel_math.h"

namespace dgs {

#ifndef DGS_FWD_MINWAVES
#define DGS_FWD_MINWAVES 5   // (the long-tile path's extra state must not cost the short path its fifth wave per SIMD)
#endif

struct BlendFwdArgs {
    const uint2* ranges;         // [T]
    const uint32_t* order;       // [T] dispatch order (mode 3) or null
    const uint32_t* point_list;  // [R] sorted surfel ids
    const float4* rec;           // [P*5]
    int W, H, tiles_x, tiles_y, mode;
    const float* bg;             // [3] device
    float* final_T;              // [3][T*256] tile-major: T, dist1, dist2
    uint32_t* n_contrib;         // [2][T*256] tile-major: last contributor, median contributor
    uint32_t* tile_last;         // [T] max over the tile of `last contributor` (zeroed by scan_tiles_kernel, written with atomicMax)
    const LongThr* long_thr;     // thresholds of the long-tile path, or null (path off: grid = blend_grid_size)
    float* out_color;            // [3,H,W]
    float* out_others;           // [8,H,W]
    // accumulator rider: the first `clear_blocks` workgroups (a multiple of 8: the XCD of every tile workgroup stays what it was) zero the
    // backward's per-surfel accumulator rows -- 80 B per surfel of stores that ride under this VALU-bound kernel instead of costing the
    // backward a 10-us launch of their own -- and *clean_flag says so to prep_bwd_kernel (1 = rows are zero; the backward blend writes 0)
    float4* clear;
    uint32_t clear_n4;
    int clear_blocks;
    uint32_t* clean_flag;
};

// ---- forward blend, one list per 16-lane row (round 4) ----------------------------------------------------------------------
// Every DPP row of the wave -- one 4x4 pixel block of the quadrant (surfel_math.h lane_pixel) -- walks the list of the entries that can
// reach ITS block: while staging, a lane tests its entry against the four blocks (blocks_hit_linear: the record's pixel box, then a
// tangent-plane bound of the footprint's conic; also what decides whether the entry is staged at all; a block whose 16 pixels are all
// finished takes no more entries), the entry's planes are stored once per wave, compacted, and each block it reaches gets the slot
// number appended to its row's byte list (rank among the ballot of that block).  One wave-instruction of the visit loop then serves
// four (entry, block) pairs: lane l reads the planes of the slot its row is at (four addresses per ds_read_b128), rows that have run
// out of entries read the null slot (opacity 0: fails the alpha test), and the loop runs max-over-rows(list length) times.  In the
// forward nothing is summed across lanes and nothing is added to global memory, so the design pays here (the same design lost in the
// backward: DESIGN.md section 4).  Per-pixel arithmetic and entry order are those of the one-list-per-wave forward of round 3 that it
// replaced (0.126 -> 0.120 ms): the results are bit-identical.  0.87 of that kernel's visits on the 200k / 800x800 scene
// (tools/blend_stats.py).

constexpr int kChunkF = 64;          // entries staged per wave and step by the row kernel: one per lane
constexpr int kNullSlotF = kChunkF;  // the slot behind the staged ones: planes of an entry that fails the alpha test for every pixel
struct FwdRowStage {
    f32x4 a[3][kChunkF + 1];
    f32x4 tw[kChunkF + 1];     // (Tw.x Tw.y Tw.z, 1-based list position as bits)
    f32x4 q3[kChunkF + 1];     // (n.x n.y n.z r)
    f32x4 q4[kChunkF + 1];     // (g b - -)
    uint32_t idx[4][17];       // row r: the slots of its block's entries in list order, one byte each (68: the loop reads two ahead of a full list)
};

// ---- forward, long tile: one quadrant per workgroup, the list in ROUNDS of four chunks ---------------------------------------
// Wave w of the workgroup takes chunk 4 r + w of round r (64 list entries).  Per round: stage the chunk once; pass 1 over the staged
// entries = alpha only, product of (1 - alpha) per pixel -> LDS, barrier; T_in of the wave = T at the start of the round x the
// products of the waves in front of it; pass 2 over the SAME staged entries = the short path's blend from T_in; the round's weights
// and distortion sums -> LDS, barrier; every wave adds the cross terms of the distortion (its entries against the running sums of
// everything in front of them, which enter linearly) and takes T behind the round from the last wave.  The walk ends like the serial
// one, when no pixel of the quadrant takes entries any more -- a quarter-per-wave split of the WHOLE list (the first version) walked
// the list behind the saturation point as well: 3.6 x slower than the serial kernel on an opaque knot (40 k surfels on a few tiles).
enum FwdLongSlot { kLPC0, kLPC1, kLPC2, kLPD, kLPN0, kLPN1, kLPN2, kLPdist, kLPT, kLPmedd, kLPmedw, kLPlast, kLPmedc, kLPCount };
struct FwdLongPart { float v[kLPCount][64]; };            // a wave's state per pixel for the final combine (aliases the staging slices)
static_assert(sizeof(FwdLongPart) <= sizeof(FwdRowStage), "the partial states alias the staging slices");
struct FwdLongX { float P[4][64], W[4][64], d1[4][64], d2[4][64]; unsigned long long done[4]; };   // one round's exchange (single copy: the
// products are read between the round's two barriers and next written behind the second one; the other arrays the other way round)

__device__ __forceinline__ void blend_fwd_long(const BlendFwdArgs& a, int tile, int q, FwdRowStage* s_stage /*[4]*/, FwdLongX& X)
{
    const int ntiles = a.tiles_x * a.tiles_y;
    const int tid = threadIdx.x, lane = tid & 63, seg = tid >> 6;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    int lx_, ly_;
    lane_pixel(64 * q + lane, lx_, ly_);
    const int px = tx * kTileX + lx_, py = ty * kTileY + ly_;
    const bool inside = px < a.W && py < a.H;
    const float tpx = (float)(tx * kTileX), tpy = (float)(ty * kTileY);
    const float X0 = tpx + 8.0f, Y0 = tpy + 8.0f;
    const float qx = tpx + (float)(8 * (q & 1)), qy = tpy + (float)(8 * (q >> 1));
    const float qus0 = kSqrt2 * ((q & 1) ? 0.5f : -7.5f), qvs0 = kSqrt2 * ((q & 2) ? 0.5f : -7.5f);
    const float us_px = inside ? kSqrt2 * ((float)lx_ - 7.5f) : __builtin_nanf("");
    const float vs = kSqrt2 * ((float)ly_ - 7.5f);
    const uint2 range = a.ranges[tile];
    const uint32_t len = range.y - range.x;
    FwdRowStage& S = s_stage[seg];

    PixFwd st;
    pixfwd_init(st);
    float T_round = 1.0f;        // T in front of the current round (pixels that still take entries)
    float T_final = 1.0f;        // T behind this wave's last blend
    float d1_tot = 0.f, d2_tot = 0.f;   // the distortion's running sums in front of the current round (the same in all four waves)
    bool done_pix = !inside;     // saturated (forward.cu:402-406) in some wave's chunk, or outside the image

    uint32_t id_next = 64u * (uint32_t)seg + (uint32_t)lane < len ? a.point_list[range.x + 64u * seg + lane] : 0u;
    for (uint32_t base = 0; base < len; base += 4 * kChunk) {
        const uint32_t e_mine = base + 64u * (uint32_t)seg + (uint32_t)lane;
        const uint32_t id = id_next;
        id_next = e_mine + 4 * kChunk < len ? a.point_list[range.x + e_mine + 4 * kChunk] : 0u;
        // stage the wave's chunk (one list for the whole quadrant here: the entries that can touch it, compacted)
        const float4* src = a.rec + (size_t)id * kRecQuads;
        const float4 q0 = src[0], q1 = src[1], q2 = src[2], q3r = src[3], q4r = src[4], bx = src[5];
        const TileAffine ta = tile_affine(as_quad(q0), as_quad(q1), as_quad(q2), X0, Y0);
        const bool hit = (e_mine < len) & block_box_hit(bx, qx, qy) & block_hit_affine(ta, qus0, qus0 + 7.0f * kSqrt2, qvs0, qvs0 + 7.0f * kSqrt2);
        const unsigned long long m = ballot64(hit);
        if (hit) {
            const int slot = lane_rank(m);
            S.a[0][slot] = mk4(ta.a0.x, ta.a0.y, ta.a0.z, ta.a0.w);
            S.a[1][slot] = mk4(ta.a1.x, ta.a1.y, ta.a1.z, ta.a1.w);
            S.a[2][slot] = mk4(ta.a2.x, ta.a2.y, ta.a2.z, ta.a2.w);
            S.tw[slot] = mk4(q1.z, q1.w, q2.x, __uint_as_float(e_mine + 1u));
            S.q3[slot] = mk4(q3r);
            S.q4[slot] = mk4(q4r);
        }
        __builtin_amdgcn_wave_barrier();
        const int nhit = __builtin_popcountll(m);
        // ---- pass 1: the chunk's product of (1 - alpha) over the entries that pass the alpha and near tests
        float P = 1.0f;
        {
            f32x4 a0 = S.a[0][0], a1 = S.a[1][0], a2 = S.a[2][0], tw = S.tw[0];
            for (int i = 0; i < nhit; i++) {
                AlphaEval e;
                const bool pass = alpha_affine(us_px, vs, as_quad(a0), as_quad(a1), as_quad(a2), e);
                asm volatile("" : "+v"(e.a), "+v"(e.alpha) : : "memory");
                a0 = S.a[0][i + 1]; a1 = S.a[1][i + 1]; a2 = S.a[2][i + 1];
                bool use3d;
                const float depth = alpha_depth(e, tw.x, tw.y, tw.z, use3d);
                const float ae = (pass & (depth >= kNear)) ? e.alpha : 0.0f;
                P = P - ae * P;
                tw = S.tw[i + 1];
            }
        }
        X.P[seg][lane] = P;
        __syncthreads();
        float T_in = T_round, T_in3 = T_round;    // T in front of this wave's chunk / of the last wave's
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float Pj = X.P[j][lane];
            T_in = j < seg ? T_in * Pj : T_in;
            T_in3 *= Pj;
        }
        // ---- pass 2: the short path's blend of the same staged entries, from T_in
        float us = (!done_pix && T_in >= kTmin) ? us_px : __builtin_nanf("");   // (a pixel below 1e-4 blends nothing: test_T <= T)
        const bool took = us == us;
        const uint32_t last_before = st.last;
        st.T = T_in;
        st.dist1 = 0.f; st.dist2 = 0.f;    // the round's own sums; the sums in front of the chunk are added in below
        if (ballot64(took) != 0ull) {
            f32x4 a0 = S.a[0][0], a1 = S.a[1][0], a2 = S.a[2][0];
            f32x4 tw = S.tw[0], q3 = S.q3[0], q4 = S.q4[0];
            for (int i = 0; i < nhit; i++) {
                AlphaEval e;
                const bool pass = alpha_affine(us, vs, as_quad(a0), as_quad(a1), as_quad(a2), e);
                asm volatile("" : "+v"(e.a), "+v"(e.alpha) : : "memory");
                a0 = S.a[0][i + 1]; a1 = S.a[1][i + 1]; a2 = S.a[2][i + 1];
                bool use3d;
                const float depth = alpha_depth(e, tw.x, tw.y, tw.z, use3d);
                float w, test_T;
                pixfwd_weight(st, e.alpha, w, test_T);
                const bool ok = pass & (depth >= kNear);
                const bool blend = ok & !(test_T < kTmin);
                if (blend) {
                    st.contributor = __float_as_uint(tw.w);
                    pixfwd_accumulate<true>(st, w, test_T, depth, as_quad(q3), Quad{q4.x, q4.y, 0.f, 0.f});
                }
                us = (ok ^ blend) ? __builtin_nanf("") : us;
                asm volatile("" : "+v"(st.T), "+v"(us) : : "memory");
                tw = S.tw[i + 1]; q3 = S.q3[i + 1]; q4 = S.q4[i + 1];
            }
        }
        __builtin_amdgcn_wave_barrier();
        const float W_own = T_in - st.T, d1_own = st.dist1, d2_own = st.dist2;   // (T only moves by the blending weights)
        X.W[seg][lane] = W_own; X.d1[seg][lane] = d1_own; X.d2[seg][lane] = d2_own;
        const unsigned long long sat = ballot64(took && !(us == us));   // pixels that saturated in this chunk
        if (lane == 0) X.done[seg] = sat;
        if (st.last != last_before) T_final = st.T;
        __syncthreads();
        // distortion (forward.cu:413-417): err_i = m_i^2 A_i + dist2_i - 2 m_i dist1_i with the running sums of ALL earlier entries; the
        // chunk used its own sums, everything in front of it enters linearly
        float p1 = d1_tot, p2 = d2_tot;
        for (int j = 0; j < seg; j++) { p1 += X.d1[j][lane]; p2 += X.d2[j][lane]; }
        st.distortion += p2 * W_own - 2.0f * p1 * d1_own;
#pragma unroll
        for (int j = 0; j < 4; j++) { d1_tot += X.d1[j][lane]; d2_tot += X.d2[j][lane]; }
        const unsigned long long any_sat = X.done[0] | X.done[1] | X.done[2] | X.done[3];
        done_pix = done_pix | (((any_sat >> lane) & 1ull) != 0ull);
        T_round = T_in3 - X.W[3][lane];   // T behind the last wave's chunk (its T_in minus its weights: the operation it performed)
        if (ballot64(!done_pix && T_round >= kTmin) == 0ull) break;   // (the same verdict in all four waves: same data)
    }

    __syncthreads();   // every wave is done with its staging slice: the waves' states go there
    FwdLongPart* part = reinterpret_cast<FwdLongPart*>(s_stage);
    {
        float (*v)[64] = part[seg].v;
        v[kLPC0][lane] = st.C[0]; v[kLPC1][lane] = st.C[1]; v[kLPC2][lane] = st.C[2]; v[kLPD][lane] = st.D;
        v[kLPN0][lane] = st.N[0]; v[kLPN1][lane] = st.N[1]; v[kLPN2][lane] = st.N[2];
        v[kLPdist][lane] = st.distortion; v[kLPT][lane] = T_final; v[kLPmedd][lane] = st.med_d; v[kLPmedw][lane] = st.med_w;
        v[kLPlast][lane] = __uint_as_float(st.last); v[kLPmedc][lane] = __uint_as_float(st.med_c);
    }
    __syncthreads();
    if (seg != 0) return;
    float C0 = 0.f, C1 = 0.f, C2 = 0.f, D = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f, dist = 0.f, T = 1.0f, medd = 0.f, medw = 0.f;
    uint32_t last = 0u, medc = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float (*v)[64] = part[k].v;
        C0 += v[kLPC0][lane]; C1 += v[kLPC1][lane]; C2 += v[kLPC2][lane]; D += v[kLPD][lane];
        N0 += v[kLPN0][lane]; N1 += v[kLPN1][lane]; N2 += v[kLPN2][lane]; dist += v[kLPdist][lane];
        const uint32_t lk = __float_as_uint(v[kLPlast][lane]), mk = __float_as_uint(v[kLPmedc][lane]);
        if (lk > last) { last = lk; T = v[kLPT][lane]; }                  // the wave that blended the pixel's last contributor holds its final T
        if (mk > medc) { medc = mk; medd = v[kLPmedd][lane]; medw = v[kLPmedw][lane]; }
    }
    uint32_t mx = inside ? last : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) atomicMax(&a.tile_last[tile], mx);
    const size_t plane = (size_t)ntiles * kTilePix;
    const size_t slot = (size_t)tile * kTilePix + 64 * q + lane;
    a.final_T[slot] = T;
    a.final_T[plane + slot] = d1_tot;
    a.final_T[2 * plane + slot] = d2_tot;
    a.n_contrib[slot] = last;
    a.n_contrib[plane + slot] = medc;
    if (inside) {
        const size_t HW = (size_t)a.H * a.W;
        const size_t pix = (size_t)py * a.W + px;
        a.out_color[pix] = C0 + T * a.bg[0];
        a.out_color[HW + pix] = C1 + T * a.bg[1];
        a.out_color[2 * HW + pix] = C2 + T * a.bg[2];
        a.out_others[pix] = D;
        a.out_others[HW + pix] = 1.f - T;
        a.out_others[2 * HW + pix] = N0;
        a.out_others[3 * HW + pix] = N1;
        a.out_others[4 * HW + pix] = N2;
        a.out_others[5 * HW + pix] = medd;
        a.out_others[6 * HW + pix] = dist;
        a.out_others[7 * HW + pix] = medw;
    }
}

__global__ void __launch_bounds__(kTilePix, DGS_FWD_MINWAVES) blend_fwd_rows_kernel(BlendFwdArgs a)
{
    __shared__ FwdRowStage s_stage[4];
    __shared__ uint32_t s_max[4];
    __shared__ FwdLongX s_x;      // long tiles: the rounds' exchange

    if (a.clean_flag && blockIdx.x == 0 && threadIdx.x == 0) *a.clean_flag = a.clear_blocks > 0 ? 1u : 0u;   // read after this launch has ended
    if ((int)blockIdx.x < a.clear_blocks) {   // accumulator rider (BlendFwdArgs)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t i = blockIdx.x * kTilePix + threadIdx.x; i < a.clear_n4; i += (uint32_t)a.clear_blocks * kTilePix) a.clear[i] = z;
        return;
    }
    const int bid = (int)blockIdx.x - a.clear_blocks;
    const int ntiles = a.tiles_x * a.tiles_y;
    int tile;
    if (a.long_thr) {   // tile order 3 with the long-tile path: see long_decode
        int lq;
        if (!long_decode(bid, a.order, ntiles, a.long_thr->fwd, nullptr, a.ranges, tile, lq)) return;
        if (lq >= 0) {
            blend_fwd_long(a, tile, lq, s_stage, s_x);
            return;
        }
    } else {
        tile = tile_for_block(bid, a.tiles_x, a.tiles_y, a.mode);
        if (a.mode < 3 && tile >= ntiles) return;
        if (a.mode >= 3) tile = (int)a.order[tile];
        if (tile >= ntiles) return;   // mode 4: empty slot
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane >> 4;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    int lx_, ly_;
    lane_pixel(tid, lx_, ly_);
    const int px = tx * kTileX + lx_, py = ty * kTileY + ly_;
    const bool inside = px < a.W && py < a.H;
    const float tpx = (float)(tx * kTileX), tpy = (float)(ty * kTileY);
    const float X0 = tpx + 8.0f, Y0 = tpy + 8.0f;
    const float qx = tpx + (float)(8 * (wave & 1)), qy = tpy + (float)(8 * (wave >> 1));
    const float qus0 = kSqrt2 * ((wave & 1) ? 0.5f : -7.5f), qvs0 = kSqrt2 * ((wave & 2) ? 0.5f : -7.5f);
    float us = inside ? kSqrt2 * ((float)lx_ - 7.5f) : __builtin_nanf("");   // NaN = this pixel takes no further entry
    const float vs = kSqrt2 * ((float)ly_ - 7.5f);

    const uint2 range = a.ranges[tile];
    const uint32_t len = range.y - range.x;
    FwdRowStage& S = s_stage[wave];
    if (lane < 6) {   // the null slot: opacity 0 (alpha = 0 * G fails the test, also for G = NaN), everything else finite
        f32x4* planes[6] = {&S.a[0][kNullSlotF], &S.a[1][kNullSlotF], &S.a[2][kNullSlotF], &S.tw[kNullSlotF], &S.q3[kNullSlotF], &S.q4[kNullSlotF]};
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (lane == k) *planes[k] = mk4(0.f, 0.f, 0.f, 0.f);
    }
    const uint8_t* my_list = (const uint8_t*)&S.idx[row][0];

    PixFwd st;
    pixfwd_init(st);

    // Visit, in list order, the entries the wave has staged.  Every instruction of this loop is issued once per visit, scalar ones
    // included (the CU's scalar unit issues ~1 instruction per cycle for all four SIMDs: 25 scalar instructions per visit -- bit-scan
    // of a visit mask, saturation ballots, early-out tests -- cost as much issue time as the arithmetic).  Hence: the staged entries
    // are COMPACTED (a counted loop), a pixel that saturates (forward.cu:402-406: it blends neither this entry nor any later one) is
    // poisoned with one select, and whether the wave still has live pixels is tested per chunk, not per visit.
    auto visit = [&](auto track_median, int niter) {
        int sl = my_list[0];
        int sl_next = my_list[1];
        f32x4 a0 = S.a[0][sl], a1 = S.a[1][sl], a2 = S.a[2][sl];
        f32x4 tw = S.tw[sl], q3 = S.q3[sl], q4 = S.q4[sl];
        for (int i = 0; i < niter; i++) {
            AlphaEval e;
            const bool pass = alpha_affine(us, vs, as_quad(a0), as_quad(a1), as_quad(a2), e);
            // Software pipeline over the visited entries with ONE register set: the next entry's alpha part is requested as soon
            // as this one's has been consumed, its Tw / normal / colour at the end of the visit -- each INTO THE SAME registers,
            // a good hundred cycles before it is needed.  The empty asm statements pin the order: left alone the compiler hoists
            // the loads above the evaluation, needs a second register set and pays twelve moves per visit to rotate it.
            asm volatile("" : "+v"(e.a), "+v"(e.alpha) : : "memory");
            sl = sl_next;
            a0 = S.a[0][sl]; a1 = S.a[1][sl]; a2 = S.a[2][sl];
            bool use3d;
            const float depth = alpha_depth(e, tw.x, tw.y, tw.z, use3d);
            float w, test_T;
            pixfwd_weight(st, e.alpha, w, test_T);
            const bool ok = pass & (depth >= kNear);      // forward.cu:388
            const bool blend = ok & !(test_T < kTmin);
            if (blend) {
                st.contributor = __float_as_uint(tw.w);   // 1-based list position (forward.cu:356)
                pixfwd_accumulate<decltype(track_median)::value>(st, w, test_T, depth, as_quad(q3), Quad{q4.x, q4.y, 0.f, 0.f});
            }
            us = (ok ^ blend) ? __builtin_nanf("") : us;   // passed but saturated: the pixel is finished
            asm volatile("" : "+v"(st.T), "+v"(us) : : "memory");
            tw = S.tw[sl]; q3 = S.q3[sl]; q4 = S.q4[sl];
            sl_next = my_list[i + 2];
            asm volatile("" : "+v"(sl_next));   // requested here, a visit before the address is formed from it
        }
    };

    uint32_t id_next = (uint32_t)lane < len ? a.point_list[range.x + lane] : 0u;
    unsigned long long alive = ballot64(inside);   // lanes that still take entries
    for (uint32_t base = 0; base < len && alive != 0ull; base += kChunkF) {
        const uint32_t e_mine = base + (uint32_t)lane;
        const uint32_t id = id_next;   // (lanes beyond the end of the list hold id 0: a valid record, masked out below)
        // Straight-line staging: all six quads of the record are requested at once and every lane runs the whole test (a
        // conditional ladder -- list end, box, footprint -- makes the compiler sink each load behind the test before it:
        // five dependent trips to memory per chunk).  Entries that can touch the quadrant are compacted: slot = rank among them.
        const float4* src = a.rec + (size_t)id * kRecQuads;
        const float4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3], q4 = src[4], bx = src[5];
        // the id of the lane's next entry travels while this chunk is visited (the record loads of the next step then start at once)
        id_next = e_mine + kChunkF < len ? a.point_list[range.x + e_mine + kChunkF] : 0u;
        const TileAffine ta = tile_affine(as_quad(q0), as_quad(q1), as_quad(q2), X0, Y0);
        uint32_t bm = e_mine < len ? blocks_hit_linear(ta, qus0, qvs0, as_quad(bx), qx, qy) : 0u;
        // a block whose pixels are all finished takes no more entries
        bm &= (((uint32_t)alive & 0xffffu) ? 1u : 0u) | (((uint32_t)(alive >> 16) & 0xffffu) ? 2u : 0u) |
              (((uint32_t)(alive >> 32) & 0xffffu) ? 4u : 0u) | (((uint32_t)(alive >> 48) & 0xffffu) ? 8u : 0u);
        const bool hit = bm != 0u;
        const unsigned long long m = ballot64(hit);
        if (m == 0ull) continue;
        const unsigned long long m0 = ballot64((bm & 1u) != 0u), m1 = ballot64((bm & 2u) != 0u), m2 = ballot64((bm & 4u) != 0u), m3 = ballot64((bm & 8u) != 0u);
        ((uint32_t*)&S.idx[0][0])[lane] = 0x01010101u * (uint32_t)kNullSlotF;   // every list: null slots behind its entries
        if (lane < 4) ((uint32_t*)&S.idx[0][0])[64 + lane] = 0x01010101u * (uint32_t)kNullSlotF;
        if (hit) {
            const int slot = lane_rank(m);
            S.a[0][slot] = mk4(ta.a0.x, ta.a0.y, ta.a0.z, ta.a0.w);
            S.a[1][slot] = mk4(ta.a1.x, ta.a1.y, ta.a1.z, ta.a1.w);
            S.a[2][slot] = mk4(ta.a2.x, ta.a2.y, ta.a2.z, ta.a2.w);
            S.tw[slot] = mk4(q1.z, q1.w, q2.x, __uint_as_float(e_mine + 1u));
            S.q3[slot] = mk4(q3);
            S.q4[slot] = mk4(q4);
            uint8_t* lists = (uint8_t*)&S.idx[0][0];
            if (bm & 1u) lists[lane_rank(m0)] = (uint8_t)slot;
            if (bm & 2u) lists[68 + lane_rank(m1)] = (uint8_t)slot;
            if (bm & 4u) lists[136 + lane_rank(m2)] = (uint8_t)slot;
            if (bm & 8u) lists[204 + lane_rank(m3)] = (uint8_t)slot;
        }
        __builtin_amdgcn_wave_barrier();   // the slice is private to this wave: its LDS writes above are ordered before its reads below
        const int n01 = max(__builtin_popcountll(m0), __builtin_popcountll(m1)), n23 = max(__builtin_popcountll(m2), __builtin_popcountll(m3));
        const int niter = __builtin_amdgcn_readfirstlane(max(n01, n23));
        // median bookkeeping (forward.cu:421-425) only while some pixel of the wave still has T > 0.5
        if (ballot64(st.T > 0.5f && us == us) != 0ull) visit(std::true_type{}, niter);
        else visit(std::false_type{}, niter);
        __builtin_amdgcn_wave_barrier();
        alive = ballot64(us == us);   // wave-level early out (forward.cu:334-336 votes per block)
    }

    // per-tile maximum of the last contributor: the backward starts there instead of walking the
    // whole list (backward.cu:276-279 skips those entries one by one)
    uint32_t mx = inside ? st.last : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        uint32_t o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) s_max[wave] = mx;
    __syncthreads();
    if (tid == 0) {
        uint32_t mm = s_max[0];
        mm = s_max[1] > mm ? s_max[1] : mm;
        mm = s_max[2] > mm ? s_max[2] : mm;
        mm = s_max[3] > mm ? s_max[3] : mm;
        a.tile_last[tile] = mm;
    }

    const size_t plane = (size_t)ntiles * kTilePix;
    const size_t slot = (size_t)tile * kTilePix + tid;
    a.final_T[slot] = st.T;
    a.final_T[plane + slot] = st.dist1;
    a.final_T[2 * plane + slot] = st.dist2;
    a.n_contrib[slot] = st.last;
    a.n_contrib[plane + slot] = st.med_c;
    if (inside) {
        const size_t HW = (size_t)a.H * a.W;
        const size_t pix = (size_t)py * a.W + px;
        a.out_color[pix] = st.C[0] + st.T * a.bg[0];
        a.out_color[HW + pix] = st.C[1] + st.T * a.bg[1];
        a.out_color[2 * HW + pix] = st.C[2] + st.T * a.bg[2];
        a.out_others[pix] = st.D;                 // DEPTH_OFFSET 0   (auxiliary.h:25-30)
        a.out_others[HW + pix] = 1.f - st.T;      // ALPHA_OFFSET 1
        a.out_others[2 * HW + pix] = st.N[0];     // NORMAL_OFFSET 2..4
        a.out_others[3 * HW + pix] = st.N[1];
        a.out_others[4 * HW + pix] = st.N[2];
        a.out_others[5 * HW + pix] = st.med_d;    // MIDDEPTH_OFFSET 5
        a.out_others[6 * HW + pix] = st.distortion;  // DISTORTION_OFFSET 6
        a.out_others[7 * HW + pix] = st.med_w;    // MEDIAN_WEIGHT_OFFSET 7
    }
}

}  // namespace dgs
